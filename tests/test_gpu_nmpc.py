"""Nonlinear MPC on the device (kp_nmpc_step, kp_lift_jacobian) against the host restatement of tests/test_nmpc_host.py
and the stored closed loop res_nonlin of example_control.m (tests/golden/arm_nmpc.npz)."""
import os

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from test_gpu_fit import make_basis
from test_nmpc_host import GOLDEN, HostNmpc, arm_nonlinear_model, load_nmpc_golden

pytestmark = pytest.mark.gpu

R_ARM = 0.1 * np.array([3e-2, 2e-2, 1e-2])


def synth(nz, m, Ns=400, seed=0):
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(-1, 1, (Ns, nz)); u = rng.uniform(-1, 1, (Ns, m))
    Mx = rng.standard_normal((nz + m, nz)) * 0.3
    beta = np.clip(alpha + 0.05 * np.tanh(np.hstack([alpha, u]) @ Mx), -1, 1)
    return {"alpha": alpha, "beta": beta, "u": u}


JAC_CASES = [
    (["poly"], [3], 4, 2),            # nvars = 6 <= 8
    (["poly"], [3], 6, 3),            # nvars = 9 > 8: the general monomial path (the arm)
    (["hermite"], [3], 3, 2),
    (["fourier"], [1], 2, 1),
    (["fourier_sparser"], [2], 3, 2),
    (["gaussian"], [6], 3, 2),
    (["poly", "fourier"], [2, 1], 2, 1),
]


@pytest.mark.parametrize("dim_red", [False, True])
@pytest.mark.parametrize("obs,deg,nz,m", JAC_CASES)
def test_lift_jacobian_matches_central_differences(ctx, obs, deg, nz, m, dim_red):
    pairs = synth(nz, m, seed=nz + m)
    rng = np.random.default_rng(1)
    nv = nz + m
    centres = [rng.uniform(-1, 1, (nv, d)) for o, d in zip(obs, deg) if o == "gaussian"]
    dic = ko.build_dictionary("nonlinear", nz, m, obs, deg, pairs, dim_red=dim_red, gaussian_centres=centres or None)
    basis = make_basis(ctx, dic)
    V = rng.uniform(-0.9, 0.9, (5, nv))
    J = ctx.lift_jacobian(basis, V)
    assert J.shape == (5, dic.N, nv)
    h = 1e-5
    for r in range(5):
        P = np.vstack([V[r] + h * e for e in np.eye(nv)] + [V[r] - h * e for e in np.eye(nv)])
        E = ko.econ_full(dic, P)
        Jfd = ((E[:nv] - E[nv:]) / (2 * h)).T
        scale = max(1.0, np.abs(Jfd).max())
        assert np.abs(J[r] - Jfd).max() / scale < 1e-7, (r, np.abs(J[r] - Jfd).max())


@pytest.fixture(scope="module")
def arm_nl():
    return arm_nonlinear_model(np.load(os.path.join(GOLDEN, "arm_data.npz")))


@pytest.fixture(scope="module")
def arm_setup(ctx, arm_nl):
    dic, mdl, sc = arm_nl
    basis = make_basis(ctx, dic)
    ref = np.load(os.path.join(GOLDEN, "blockM_ref.npz"))["y"]
    ref_sc = (ref - sc["y_offset"][-2:]) / sc["y_factor"][-2:]
    return dic, mdl, sc, basis, ref_sc


def arm_nmpc(ctx, arm_setup, box=False, slope=True, smooth=False, sb=None, tol=1e-9, max_iter=100, tol_step=1e-6):
    dic, mdl, sc, basis, _ = arm_setup
    lo = hi = None
    if box:
        lo = (-7 * np.pi / 8 - sc["u_offset"]) / sc["u_factor"]; hi = (7 * np.pi / 8 - sc["u_offset"]) / sc["u_factor"]
    sl = 1e-1 * sc["u_factor"].mean() if slope else None
    sm = 0.05 ** 2 * 1e-1 * sc["u_factor"].mean() if smooth else None
    dev = kra.Nmpc(ctx, basis, mdl["Kf"], 10, np.eye(6)[-2:], 10.0, 100.0, R_ARM, lo, hi, sl, sm)
    dev.set_options(max_iter, tol, tol_step)
    host = HostNmpc(dic, mdl["Kf"], 10, np.eye(6)[-2:], 10.0, 100.0, R_ARM, lo, hi, sl, sm)
    if sb is not None:
        dev.set_state_bounds(*sb)
        host.sb_lo, host.sb_hi = sb
    return dev, host


@pytest.mark.parametrize("case", ["box+slope", "slope+smooth", "state_bounds"])
def test_arm_step_matches_host_restatement(ctx, arm_setup, case):
    """One step at stored states, solved to tight tolerance: the device optimum equals the host's (SLSQP, polished on its
    active set) to 1e-6, the device's KKT residual is within its tolerance, every constraint holds to 1e-9 and, with state
    bounds, a bound is active at the optimum."""
    dic, mdl, sc, basis, ref_sc = arm_setup
    d = load_nmpc_golden()
    ysc = lambda y: ko.scaledown(sc, "y", y)
    usc = lambda u: ko.scaledown(sc, "u", u)
    sb = None
    if case == "state_bounds":        # bounds on every state that bind along the stored motion
        Ys = ysc(d["Y"])
        sb = (Ys.min(axis=0) - 0.02, Ys.max(axis=0) - 0.05)
    tol = 1e-8 if sb is not None else 1e-10
    dev, host = arm_nmpc(ctx, arm_setup, box=case == "box+slope", smooth=case == "slope+smooth", sb=sb, tol=tol, max_iter=400,
                         tol_step=1e-8)
    for k in (SB_STEPS if sb is not None else (40, 120, 200)):
        zeta, up, Yr = ysc(d["Y"][k]), usc(d["U"][k]), ref_sc[k:k + 11].ravel()
        if sb is not None:
            zeta = np.clip(zeta, sb[0] + 1e-3, sb[1] - 1e-3)          # (z_0 itself must satisfy the bounds)
        U, Z, info, st = dev.step(zeta, up, Yr)
        Uh, res = host.solve(zeta, up, Yr)
        dU = np.abs(U - Uh).max()
        nact = 0 if sb is None else int(((Z <= sb[0] + 1e-8) | (Z >= sb[1] - 1e-8)).sum())
        print(f"{case} k={k}: status {st}, |U_dev - U_host| = {dU:.2e}, SQP iterations {int(info[0])}, KKT {info[1]:.1e}, "
              f"active state bounds {nact}")
        Jd, Jh = host.cost(zeta, U, Yr), host.cost(zeta, Uh, Yr)
        print(f"    cost device {Jd:.12e} host {Jh:.12e}")
        if case == "slope+smooth" and st == F.KP_ERR_NOT_CONVERGED:
            # measured limit: with active smooth rows the iteration can converge linearly - 400 iterations
            # end at a KKT residual of 1.1e-8 (stored step 40, 4.4e-8 from the host optimum) and 4.5e-8 (step 120, 5.9e-6)
            assert info[1] <= 1e-7, info
            assert dU < 1e-5 and Jd <= Jh * (1 + 1e-10), (k, dU, Jd, Jh)
        else:
            assert st == F.KP_OK, (k, st, info)
            assert info[1] <= tol, info
        if sb is not None:
            # with binding state bounds the problem has several KKT points: the device's must be at least as good as the
            # one the host reached from the same start
            assert Jd <= Jh * (1 + 1e-9), (k, Jd, Jh)
        elif st == F.KP_OK:
            assert dU < 1e-6, (k, dU, res.message)
        assert np.array_equal(U[0], up)
        Zh, _ = host.rollout(zeta, U)
        assert np.abs(Z - Zh).max() < 1e-10
        if host.lo is not None:
            assert (U >= host.lo - 1e-9).all() and (U <= host.hi + 1e-9).all()
        assert np.abs(np.diff(U, axis=0)).max() <= host.slope + 1e-9
        if host.smooth is not None:
            assert np.abs(U[:-2] - 2 * U[1:-1] + U[2:]).max() <= host.smooth + 1e-9
        if sb is not None:
            assert (Z >= sb[0] - 1e-9).all() and (Z <= sb[1] + 1e-9).all()
            assert nact > 0, k


# a stored state whose z_1 (fixed by u_1 = u_prev) lies inside the bounds (at step 100 it does not: KP_ERR_QP_FAIL, rightly).
# Measured there: the device optimum's cost is 0.12875, the host SLSQP's (another KKT point, same start) 0.13682.
SB_STEPS = (40,)


def test_step_jacobians_are_the_lift_jacobians(ctx, arm_setup):
    dic, mdl, sc, basis, ref_sc = arm_setup
    d = load_nmpc_golden()
    dev, _ = arm_nmpc(ctx, arm_setup)
    zeta, up = ko.scaledown(sc, "y", d["Y"][60]), ko.scaledown(sc, "u", d["U"][60])
    U, Z, info, st = dev.step(zeta, up, ref_sc[60:71].ravel())
    assert st == F.KP_OK
    AB = dev.last_jacobians()
    V = np.hstack([Z[:-1], U])
    J = ctx.lift_jacobian(basis, V)
    for k in range(10):
        ref = mdl["Kf"] @ J[k]
        assert np.abs(AB[k] - ref).max() < 1e-11 * max(1.0, np.abs(ref).max()), k


@pytest.fixture(scope="module")
def arm_ks(ctx):
    g = np.load(os.path.join(GOLDEN, "arm_data.npz"))
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    return kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="nonlinear", obs_type=["poly"], obs_degree=[3],
                      snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()


def make_arm(golden):
    g = golden["arm_plant"]
    params = {k[2:]: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files if k.startswith("p_")}
    return kra.Arm(params, output_type="markers")


def example_kmpc(ks, **kw):
    args = dict(horizon=10, input_bounds=[], input_slopeConst=1e-1, input_smoothConst=None, state_bounds=[], cost_running=10,
                cost_terminal=100, cost_input=R_ARM, projmtx=ks.model["C"][-2:, :], mpc_type="nonlinear")
    args.update(kw)
    return kra.Kmpc(ks, **args)


def test_stored_nonlinear_run_replayed_teacher_forced_on_device(ctx, arm_ks):
    """All 299 steps of res_nonlin: at step k the controller sees the stored Y(k), U(k) and the reference rows k..k+10
    and returns the stored U(k+1) (fmincon's stopping tolerances set the deviation).  Measured on the MI355X at tol 1e-9:
    median 2.9e-5, max 5.1e-4 (step 29), step 0 (from rest) 4.5e-8; SQP iterations median 21, 5 steps at the cap of 100."""
    ks = arm_ks
    d = load_nmpc_golden()
    ref = np.load(os.path.join(GOLDEN, "blockM_ref.npz"))["y"]
    mpc = example_kmpc(ks, nmpc_tol=1e-9, nmpc_max_iter=100)
    ref_sc = mpc.scaledown_ref(ref)
    dev = np.empty(299); its = np.empty(299); sts = np.empty(299, dtype=int)
    for k in range(299):
        cur = {"y": ks.scaledown_y(d["Y"][k])[None, :], "u": ks.scaledown_u(d["U"][k])[None, :]}
        U, z = mpc.get_mpcInput_nonlinear(cur, ref_sc[k:k + 11])
        assert not np.isnan(U).any()
        assert np.array_equal(z[6:], np.zeros(82)) and np.allclose(z[:6], cur["y"][0])
        dev[k] = np.abs(ks.scaleup_u(U[1]) - d["U"][k + 1]).max()
        its[k] = mpc.last_info[0]; sts[k] = mpc.last_info[2]
    print(f"replay: median {np.median(dev):.2e} max {dev.max():.2e} (step {dev.argmax()}), step 0 {dev[0]:.2e}; "
          f"SQP iterations median {np.median(its)} max {its.max()}; statuses {dict(zip(*np.unique(sts, return_counts=True)))}")
    assert (sts != F.KP_ERR_QP_FAIL).all()
    assert dev[0] < 1e-6, dev[0]            # from rest: fmincon's minimum (the damped first steps, kp_nmpc.hip)
    assert np.median(dev) < 4e-5, np.median(dev)
    assert dev.max() < 7e-4, dev.max()


def test_free_running_example_control_loop_on_the_arm(ctx, arm_ks, golden):
    """example_control.m's nonlinear loop on the true arm plant (block M, 300 steps), input_bounds = []: the loop stays on
    the stored run - measured: U within 1e-3 and Y within 1e-4 of res_nonlin for all 301 samples (Y to 1.8e-5), mean
    tracking error 0.0192294 against the stored 0.0192289.  With example_control.m's +-7 pi/8 box: 0.017590 (the bilinear
    loop's stored run: 0.0203)."""
    ks = arm_ks
    d = load_nmpc_golden()
    ref = golden["blockM_ref"]["y"]
    mpc = example_kmpc(ks)
    res = kra.Ksim(make_arm(golden), mpc).run_trial_mpc(ref)
    assert res["U"].shape == (301, 3)
    e = np.mean(res["err"])
    dev = np.abs(res["U"] - d["U"]).max(axis=1)
    stay = {t: int(np.argmax(dev > t)) if (dev > t).any() else len(dev) for t in (1e-6, 1e-4, 1e-3)}
    devy = np.abs(res["Y"] - d["Y"]).max(axis=1)
    stay_y = {t: int(np.argmax(devy > t)) if (devy > t).any() else len(devy) for t in (1e-6, 1e-4, 1e-3)}
    info = np.asarray(res["nmpc_info"])
    print(f"free-running: mean err {e:.6f} (stored {d['err'].mean():.6f}); U on the stored run for {stay} steps, Y for {stay_y}; "
          f"comp_time mean {1e3 * np.mean(res['comp_time']):.3f} ms; iterations max {info[:, 0].max()}, statuses "
          f"{dict(zip(*np.unique(info[:, 2], return_counts=True)))}")
    assert abs(e - d["err"].mean()) < 2e-6, e
    assert stay[1e-3] == 301 and stay_y[1e-4] == 301, (stay, stay_y)
    mpc2 = example_kmpc(ks, input_bounds=[-7 * np.pi / 8, 7 * np.pi / 8])
    res2 = kra.Ksim(make_arm(golden), mpc2).run_trial_mpc(ref)
    assert res2["U"].shape == (301, 3)
    assert np.abs(res2["U"]).max() <= 7 * np.pi / 8 + 1e-9
    e2 = np.mean(res2["err"])
    print(f"free-running, +-7 pi/8 box: mean err {e2:.6f}")
    assert abs(e2 - 0.017590) < 1e-4, e2


def test_batch_equals_single_steps_and_warm_start_reaches_the_same_optimum(ctx, arm_setup):
    """kp_nmpc_step_batch is the single step's kernel: the same bits.  A start from a perturbed shifted solution reaches
    the cold start's optimum."""
    dic, mdl, sc, basis, ref_sc = arm_setup
    d = load_nmpc_golden()
    dev, _ = arm_nmpc(ctx, arm_setup)
    ks_ = list(range(10, 290, 35))
    Z0 = np.array([ko.scaledown(sc, "y", d["Y"][k]) for k in ks_])
    UP = np.array([ko.scaledown(sc, "u", d["U"][k]) for k in ks_])
    YR = np.array([ref_sc[k:k + 11].ravel() for k in ks_])
    Ub, Zb, ib, sb_ = dev.step_batch(Z0, UP, YR)
    for i in range(len(ks_)):
        U, Z, info, st = dev.step(Z0[i], UP[i], YR[i])
        assert st == sb_[i] == F.KP_OK
        assert np.array_equal(U, Ub[i]) and np.array_equal(Z, Zb[i]) and np.array_equal(info, ib[i])
        # warm start from the solution of the previous sample, shifted
    # a start from a perturbed, shifted solution reaches the cold start's optimum (both solved to a KKT residual of 1e-11)
    dev.set_options(300, 1e-11, 1e-10)
    for i in range(len(ks_)):
        U, _, info, st = dev.step(Z0[i], UP[i], YR[i])
        Ui = np.vstack([U[1:], U[-1:]]) + 0.01
        Uw, _, iw, stw = dev.step(Z0[i], UP[i], YR[i], U_init=Ui)
        print(f"warm start {ks_[i]}: |U_warm - U_cold| = {np.abs(Uw - U).max():.1e}, iterations {info[0]} / {iw[0]}, KKT {info[1]:.1e} / {iw[1]:.1e}")
        assert st == stw == F.KP_OK, (st, stw, info, iw)
        assert np.abs(Uw - U).max() < 1e-8, np.abs(Uw - U).max()


def test_infeasible_state_bounds_give_nan_and_qp_fail(ctx, arm_setup, arm_ks, golden):
    dic, mdl, sc, basis, ref_sc = arm_setup
    d = load_nmpc_golden()
    zeta = ko.scaledown(sc, "y", d["Y"][50])
    dev, _ = arm_nmpc(ctx, arm_setup, sb=(zeta + 0.1, zeta + 0.2))     # z_0 itself violates them
    U, Z, info, st = dev.step(zeta, ko.scaledown(sc, "u", d["U"][50]), ref_sc[50:61].ravel())
    assert st == F.KP_ERR_QP_FAIL and np.isnan(U).all()
    # Ksim stops at the first failed step (Ksim.m:220-222)
    y0 = d["Y"][0]
    mpc = example_kmpc(arm_ks, state_bounds=[[y0[i] + 0.5, y0[i] + 1.0] for i in range(6)])
    res = kra.Ksim(make_arm(golden), mpc).run_trial_mpc(golden["blockM_ref"]["y"])
    assert res["U"].shape[0] == 1 and len(res["err"]) == 0


def test_refusals(ctx, arm_setup, arm_ks):
    dic, mdl, sc, basis, ref_sc = arm_setup
    pairs = synth(2, 1)
    bil = make_basis(ctx, ko.build_dictionary("bilinear", 2, 1, ["poly"], [2], pairs))
    with pytest.raises(F.KoopmanHipError, match="nonlinear model type"):
        kra.Nmpc(ctx, bil, np.zeros((2, bil.N)), 5, np.eye(2), 1.0, 1.0, [0.1])
    with pytest.raises(F.KoopmanHipError, match="<= 64"):
        kra.Nmpc(ctx, basis, mdl["Kf"], 22, np.eye(6)[-2:], 1.0, 1.0, R_ARM)
    with pytest.raises(ValueError, match="nzeta x N"):
        kra.Nmpc(ctx, basis, mdl["Kf"][:, :-1], 10, np.eye(6)[-2:], 1.0, 1.0, R_ARM)
    with pytest.raises(NotImplementedError, match="no linear MPC"):
        kra.Kmpc(arm_ks, horizon=10, projmtx=arm_ks.model["C"][-2:, :], mpc_type="linear")
    from _loaded_system import make_trials
    trials = make_trials(10, 120, nw=1, seed=3)
    ksl = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, ctx=ctx, model_type="nonlinear", obs_type=["poly"], obs_degree=[2],
                     loaded=True).train_models()
    with pytest.raises(NotImplementedError, match="loaded model"):
        kra.Kmpc(ksl, horizon=5, projmtx=np.eye(2)[:1])
    g = np.load(os.path.join(GOLDEN, "arm_data.npz"))
    tr = [{"t": g["train_t"][:200], "y": g["train_y"][:200], "u": g["train_u"][:200]}]
    ksd = kra.Ksysid({"train": tr, "val": tr}, ctx=ctx, model_type="nonlinear", obs_type=["poly"], obs_degree=[2],
                     snapshots=np.inf, lasso=[np.inf], delays=1).train_models()
    with pytest.raises(NotImplementedError, match="nd > 0"):
        kra.Kmpc(ksd, horizon=5)
    ksb = kra.Ksysid({"train": tr, "val": tr}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[2],
                     snapshots=np.inf, lasso=[np.inf], delays=0).train_models()
    with pytest.raises(NotImplementedError, match="F_sym"):
        kra.Kmpc(ksb, horizon=5, mpc_type="nonlinear")


@pytest.mark.parametrize("nz,m,Np,obs,deg", [(2, 1, 8, ["poly"], [3]), (3, 2, 6, ["hermite"], [2]),
                                             (2, 2, 5, ["gaussian"], [5]), (4, 1, 12, ["fourier_sparser"], [2])])
def test_small_random_models_match_host_restatement(ctx, nz, m, Np, obs, deg):
    pairs = synth(nz, m, Ns=600, seed=3 * nz + m)
    rng = np.random.default_rng(nz * 10 + m)
    centres = [rng.uniform(-1, 1, (nz + m, d)) for o, d in zip(obs, deg) if o == "gaussian"]
    dic = ko.build_dictionary("nonlinear", nz, m, obs, deg, pairs, dim_red=False, gaussian_centres=centres or None)
    koop = ko.get_koopman(dic, pairs)
    Kf = ko.get_nlmodel(dic, koop, nz)["Kf"]
    basis = make_basis(ctx, dic)
    proj = np.eye(nz)[:1]
    dev = kra.Nmpc(ctx, basis, Kf, Np, proj, 5.0, 50.0, np.full(m, 0.05), -0.8 * np.ones(m), 0.8 * np.ones(m), 0.3, None)
    dev.set_options(100, 1e-9, 1e-9)
    host = HostNmpc(dic, Kf, Np, proj, 5.0, 50.0, np.full(m, 0.05), -0.8 * np.ones(m), 0.8 * np.ones(m), 0.3)
    for t in range(2):
        zeta = rng.uniform(-0.5, 0.5, nz); up = rng.uniform(-0.3, 0.3, m); Yr = np.full(Np + 1, 0.4 * (-1) ** t)
        U, Z, info, st = dev.step(zeta, up, Yr)
        assert st == F.KP_OK, (st, info)
        Uh, res = host.solve(zeta, up, Yr)
        assert np.abs(U - Uh).max() < 1e-6, (np.abs(U - Uh).max(), res.message)
