"""The device arm plant (kp_arm_simulate, kra.DeviceArm) against the stored training trials, the host yardsticks
arm.ode45_span / arm.dopri45, energy conservation, batch independence, the closed loop of example_control.m and the
sysid data path.  One GPU lane per trial; see include/koopman_hip_arm.h for the modes and row rules."""
import ctypes as C

import numpy as np
import pytest

import koopman_realizations_amd as kra
from _arm_span_reference import golden_arm, host_span
from koopman_realizations_amd import _ffi as F
from koopman_realizations_amd.arm import dopri45

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def darm(golden, ctx):
    return _device_arm(golden, ctx)


def _device_arm(golden, ctx, **kw):
    a = golden_arm(golden, **kw)
    return kra.DeviceArm(a.params, "markers", ctx=ctx)


def _stored_trials(golden):
    g = golden["arm_data"]
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    return g, off


def test_stored_training_data_in_one_call(golden, darm):
    """All 10 stored trials (1 201 samples each) in ONE SPAN_ZOH launch with the stored inputs: the outputs to 1e-8
    (host restatement: 2.7e-10), the 200 stored states of trial 0 to 1e-7."""
    g, off = _stored_trials(golden)
    t = g["train_t"][:1201, 0]
    U = np.stack([g["train_u"][a:b] for a, b in zip(off[:-1], off[1:])])
    sims = darm.simulate_ode45(t, U)
    assert len(sims) == 10
    for j, (a, b) in enumerate(zip(off[:-1], off[1:])):
        assert np.abs(sims[j]["y"] - g["train_y"][a:b]).max() <= 1e-8, j
    assert np.abs(sims[0]["x"][:200] - golden["arm_plant"]["train_x"]).max() <= 1e-7
    st = darm.last_stats
    assert (st["status"] == 0).all() and (st["naccept"] > 60000).all()
    s0 = sims[0]
    assert s0["t"].shape == (1201, 1) and s0["x"].shape == (1201, 6) and s0["u"].shape == (1201, 3)
    assert s0["w"].shape == (1201, 2) and (s0["alpha"] == s0["x"][:, :3]).all() and (s0["alphadot"] == s0["x"][:, 3:]).all()


@pytest.mark.parametrize("mode", ["zoh", "interp", "floor"])
@pytest.mark.parametrize("w", [None, (0.3, 0.4)])
def test_span_modes_match_host_ode45_span(golden, ctx, mode, w):
    """40-sample slices of a stored trial in every SPAN mode, unloaded and loaded: the same accepted / rejected step
    counts as ode45_span with the same row rule, and states within 2e-9.  The bound is not looser than the host itself
    can do: the kernel's closed-form equations of motion, evaluated in numpy in place of Arm.vf, move this slice by
    8e-10 with identical step counts (ode45's step-size control feeds the rounding of its error estimate, a
    difference of nearly equal stages, into the step sizes, and the stiff arm keeps that through ~2 000 steps)."""
    g, off = _stored_trials(golden)
    arm = golden_arm(golden)
    t = g["train_t"][:40, 0]
    u = g["train_u"][off[3]:off[3] + 40]
    Xh, st = host_span(arm, t, u, w, rule=mode, Ts=0.05)
    W = None if w is None else np.broadcast_to(np.array(w), (1, 40, 2))
    X, na, nr, s = ctx.arm_simulate(arm.params, mode, t, u[None], W, Ts=0.05)
    assert s[0] == 0
    assert X.shape == (1,) + Xh.shape
    assert (na[0], nr[0]) == (st["naccept"], st.get("nreject", 0))
    assert np.abs(X[0] - Xh).max() <= 2e-9


def test_restart_mode_stored_closed_loop_transitions(golden, darm):
    """The 300 stored closed-loop transitions X(k) -> X(k+1) (Ksim.m:239-245) as one simulate_Ts_batch: to 1e-10 of the
    stored next states, step counts equal to dopri45's."""
    gp = golden["arm_plant"]
    X, U = gp["bilin_X"], gp["bilin_U"]
    X1 = darm.simulate_Ts_batch(X[:300], U[:300])
    assert np.abs(X1 - X[1:301]).max() <= 1e-10
    na, nr = darm.last_stats["naccept"], darm.last_stats["nreject"]
    arm = golden_arm(golden)
    for k in range(300):
        st = {}
        dopri45(lambda t, x: arm.vf(x, U[k], (0.0, 0.0)), 0.0, arm.params["Ts"], X[k], stats=st)
        assert (na[k], nr[k]) == (st["naccept"], st.get("nreject", 0)), k
    # the single-step entry point and the per-sample simulate give the same states
    assert np.array_equal(darm.simulate_Ts(X[7], U[7]), X1[7])
    t = np.arange(6) * 0.05
    sim = darm.simulate(t, U[:6])
    ref = kra.Arm(arm.params, "markers").simulate(t, U[:6])
    assert np.abs(sim["x"] - ref["x"]).max() <= 1e-12


@pytest.mark.parametrize("nmods,nlinks", [(3, 1), (1, 1), (2, 4)])
def test_energy_conserved_without_damping_spring_or_input(golden, ctx, nmods, nlinks):
    """d = ku = k = 0, rtol 1e-10: the total energy (test_arm_plant.py's formula) drifts at most 1e-6 over 2 s, with
    and without an end-effector load, for 3, 1 and 8 links."""
    n = nmods * nlinks
    base = golden_arm(golden).params
    p = dict(base); p.update(d=0.0, ku=0.0, k=0.0, Nmods=nmods, nlinks=nlinks, Nlinks=n, nx=2 * n, l=1.0 / n)
    free = kra.Arm(p, "markers")
    rng = np.random.default_rng(n)
    x0 = np.concatenate([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.5, 0.5, n)])
    for w in ((0.0, 0.0), (0.3, 0.4)):
        def energy(x):
            a, ad = x[:n], x[n:]
            D = free.get_massMatrix(a, w)
            xj, xcm = free.alpha2x(a)
            grav = np.array([-np.sin(w[1]), np.cos(w[1])])
            return 0.5 * ad @ D @ ad - p["m"] * p["g"] * (xcm @ grav).sum() - w[0] * p["g"] * (xj[-1] @ grav)

        t = np.linspace(0.0, 2.0, 11)
        X, na, nr, st = ctx.arm_simulate(p, "restart", t, np.zeros((1, 11, nmods)), np.broadcast_to(np.array(w), (1, 11, 2)),
                                         x0[None], rtol=1e-10, atol=1e-12)
        assert st[0] == 0
        e0 = energy(x0)
        drift = max(abs(energy(x) - e0) for x in X[0])
        assert drift <= 1e-6 * max(1.0, abs(e0)), (n, w, drift)
        assert np.abs(X[0, -1] - x0).max() > 0.05


def _mixed_batch(golden, b, T, seed):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-2, 2, (b, T, 3))
    W = np.stack([np.broadcast_to(np.array([rng.uniform(0, 0.5), rng.uniform(-1, 1)]), (T, 2)) for _ in range(b)])
    x0 = np.concatenate([rng.uniform(-1, 1, (b, 3)), rng.uniform(-2, 2, (b, 3))], axis=1)
    return U, W, x0


def test_batch_independence_and_per_trial_failure(golden, ctx):
    """A trial's result is bit-identical alone and inside a batch; batches of 1, 63, 64, 65 and 16 384 lanes (short spans)
    agree with the 1 000-trial batch on the trials they share.  A trial with a non-finite initial state fails alone:
    status KP_ERR_NOT_CONVERGED and NaN from its first output on, its neighbours untouched.  A tolerance the step
    control cannot meet fails every trial of the call."""
    p = golden_arm(golden).params
    t = np.arange(4) * 0.05
    U, W, x0 = _mixed_batch(golden, 16384, 4, 11)
    for mode in ("zoh", "restart"):
        Xb, na, nr, st = ctx.arm_simulate(p, mode, t, U[:1000], W[:1000], x0[:1000])
        assert (st == 0).all() and np.isfinite(Xb).all()
        for j in (0, 1, 63, 64, 500, 999):
            X1, na1, nr1, _ = ctx.arm_simulate(p, mode, t, U[j:j + 1], W[j:j + 1], x0[j:j + 1])
            assert np.array_equal(X1[0], Xb[j]) and na1[0] == na[j] and nr1[0] == nr[j], (mode, j)
        for b in (1, 63, 64, 65, 16384):
            Xs, _, _, sts = ctx.arm_simulate(p, mode, t, U[:b], W[:b], x0[:b])
            k = min(b, 1000)
            assert (sts == 0).all() and np.array_equal(Xs[:k], Xb[:k]), (mode, b)
        # one failing lane among its neighbours
        x0f = x0[:65].copy(); x0f[40, 2] = np.nan
        Xf, _, _, stf = ctx.arm_simulate(p, mode, t, U[:65], W[:65], x0f)
        assert stf[40] == F.KP_ERR_NOT_CONVERGED and np.isnan(Xf[40, 1:]).all()
        ok = np.arange(65) != 40
        assert (stf[ok] == 0).all() and np.array_equal(Xf[ok], Xb[:65][ok])
    # step-control failure: rtol = atol = 1e-300 cannot be met
    Xu, _, _, stu = ctx.arm_simulate(p, "zoh", t, U[:3], W[:3], x0[:3], rtol=1e-300, atol=1e-300)
    assert (stu == F.KP_ERR_NOT_CONVERGED).all() and np.isnan(Xu[:, 1:]).all() and np.array_equal(Xu[:, 0], x0[:3])


def _call(ctx, params, mode=0, batch=1, T=4, t=None, Ts=0.05, U=None, rtol=1e-3, atol=1e-6, X=None):
    t = np.arange(T) * 0.05 if t is None else np.asarray(t, dtype=np.float64)
    nm = max(params.Nmods, 1)
    U = np.zeros((batch, max(T, 1), nm)) if U is None else U
    X = np.zeros((batch, max(T, 1), 2 * max(params.Nmods * params.nlinks, 1))) if X is None else X
    st = np.zeros(batch, dtype=np.int32)
    rc = F.lib().kp_arm_simulate(ctx.handle, C.byref(params), mode, batch, T, F.dptr(t), Ts, None, F.dptr(U), None, rtol, atol,
                                 F.dptr(X), None, None, st.ctypes.data_as(F.c_ip))
    return rc, F.lib().kp_last_error(ctx.handle).decode()


def test_argument_errors(golden, ctx, darm):
    p0 = golden_arm(golden).params

    def prm(**kw):
        d = dict(Nmods=3, nlinks=1, l=p0["l"], k=p0["k"], d=p0["d"], m=p0["m"], i=p0["i"], g=p0["g"], ku=p0["ku"])
        d.update(kw)
        return F.KpArmParams(d["Nmods"], d["nlinks"], d["l"], d["k"], d["d"], d["m"], d["i"], d["g"], d["ku"])

    assert _call(ctx, prm())[0] == F.KP_OK
    assert _call(ctx, prm(Nmods=8))[0] == F.KP_OK
    bad = [dict(params=prm(Nmods=9)), dict(params=prm(Nmods=3, nlinks=3)), dict(params=prm(Nmods=0)),
           dict(params=prm(nlinks=0)), dict(params=prm(m=np.nan)), dict(params=prm(ku=np.inf)),
           dict(params=prm(), t=np.array([0.01, 0.05, 0.1, 0.15])), dict(params=prm(), t=np.array([0.0, 0.05, 0.05, 0.1])),
           dict(params=prm(), t=np.array([0.0, 0.1, 0.05, 0.2])), dict(params=prm(), T=1),
           dict(params=prm(), mode=1, T=2), dict(params=prm(), rtol=0.0), dict(params=prm(), atol=-1.0),
           dict(params=prm(), rtol=np.nan), dict(params=prm(), mode=2, Ts=0.0), dict(params=prm(), mode=2, Ts=-0.05),
           dict(params=prm(), mode=4), dict(params=prm(), mode=-1), dict(params=prm(), batch=0)]
    for kw in bad:
        p = kw.pop("params")
        rc, msg = _call(ctx, p, **kw)
        assert rc == F.KP_ERR_ARG and msg.startswith("kp_arm_simulate"), kw
    # Python argument errors, as Arm.m raises them
    t = np.arange(5) * 0.05
    u = np.zeros((5, 3))
    for call in (lambda: darm.simulate_ode45(t, u, input_type="foh"), lambda: darm.simulate_ode45(t, u[:4]),
                 lambda: darm.simulate_ode45(t, u[:, :2]), lambda: darm.simulate_ode45(t, u, np.zeros((5, 3))),
                 lambda: darm.simulate_ode45(np.zeros((5, 2)), u), lambda: darm.simulate(t, u[:4]),
                 lambda: darm.simulate(t, u[:, :2]), lambda: darm.simulate_Ts(np.zeros(6), np.zeros(3), np.zeros(3)),
                 lambda: darm.simulate_Ts_batch(np.zeros((2, 5)), np.zeros((2, 3))),
                 lambda: darm.simulate_rampNhold(1.0, 0.5, [0.1, 0.2, 0.3]), lambda: darm.simulate_rampNhold(1.0, 0.5, [0, 0], trials=0),
                 lambda: darm.get_rampNhold(1.0, 0.5, [0, 0], [1])):
        with pytest.raises(ValueError):
            call()


def _example_control(ctx, golden, plant_cls):
    """test_gpu_mpc.py's example_control.m setup (bilinear, poly-3, dim_red), with the plant class as a parameter."""
    g = golden["arm_data"]; gp = golden["arm_plant"]
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()
    mpc = kra.Kmpc(ks, horizon=10, input_bounds=[-7 * np.pi / 8, 7 * np.pi / 8], input_slopeConst=1e-1, input_smoothConst=None,
                   state_bounds=None, cost_running=10, cost_terminal=100, cost_input=0.1 * np.array([3e-2, 2e-2, 1e-2]),
                   projmtx=ks.model["C"][-2:, :])
    params = {k[2:]: (float(gp[k]) if gp[k].ndim == 0 else gp[k]) for k in gp.files if k.startswith("p_")}
    plant = kra.DeviceArm(params, "markers", ctx=ctx) if plant_cls is kra.DeviceArm else kra.Arm(params, "markers")
    return ks, kra.Ksim(plant, mpc)


def test_closed_loop_with_device_plant(ctx, golden):
    """Ksim(DeviceArm(...), kmpc).run_trial_mpc on the block-M reference equals the same loop around the host Arm to 1e-8
    in Y and tracks within test_gpu_mpc.py's bound of the stored run."""
    ref = golden["blockM_ref"]["y"]
    ks, sim_d = _example_control(ctx, golden, kra.DeviceArm)
    res_d = sim_d.run_trial_mpc(ref, None, None)
    _, sim_h = _example_control(ctx, golden, kra.Arm)
    res_h = sim_h.run_trial_mpc(ref, None, None)
    assert res_d["Y"].shape == (301, 6)
    assert np.abs(res_d["Y"] - res_h["Y"]).max() <= 1e-8
    stored = float(golden["arm_plant"]["bilin_err"].mean())
    assert 0.7 * stored < res_d["err"].mean() < 1.1 * stored


def test_sysid_data_path(ctx, golden, darm):
    """simulate_ode45 with the stored inputs gives training data that fits the same model as the stored data
    (example_sysid.m's linear poly-3 dim_red configuration): validation errors equal to 1e-6 relative.  A loaded
    simulate_rampNhold batch trains a loaded bilinear model whose validation error is finite."""
    g, off = _stored_trials(golden)
    t = g["train_t"][:1201, 0]
    sims = darm.simulate_ode45(t, [g["train_u"][a:b] for a, b in zip(off[:-1], off[1:])])
    stored = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = {"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}
    errs = []
    for train in (stored, sims):
        ks = kra.Ksysid({"train": train, "val": [val]}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[3],
                        snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()
        errs.append(ks.val_model(ks.model, val)["error"]["euclid_mean"])
    assert np.isfinite(errs[0]) and abs(errs[1] - errs[0]) <= 1e-6 * errs[0]
    rng = np.random.default_rng(5)
    loads = np.stack([rng.uniform(0.0, 0.5, 10), rng.uniform(-0.5, 0.5, 10)], axis=1)
    trials = darm.simulate_rampNhold(10.0, 1.0, loads, trials=10, rng=rng)
    assert len(trials) == 10 and trials[0]["x"].shape == (201, 6) and (trials[3]["w"] == loads[3]).all()
    assert np.abs(trials[0]["u"]).max() <= darm.params["umax"] + 1e-12
    ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[2],
                    loaded=True).train_models()
    err = ks.val_BLmodel(ks.model, trials[9])["error"]["euclid_mean"]
    assert np.isfinite(err)


def test_ramp_and_hold_signal_and_floor_rule(golden, ctx, darm):
    """get_rampNhold follows Arm.m:1054-1083 (holds between ramps, tsteps = 0 : Ts : tf); simulate_rampNhold integrates
    it with the floor(t / Ts) row, as the host yardstick does (to 2e-9: the rounding bound of
    test_span_modes_match_host_ode45_span)."""
    sig, ts = darm.get_rampNhold(2.0, 0.5, [-1, 0], [1, 2], np.random.default_rng(0))
    assert ts.shape == (41,) and ts[-1] == 2.0 and sig.shape == (41, 2)
    assert np.array_equal(sig[10], sig[0]) and (sig[:, 1] >= 0).all()
    sim = darm.simulate_rampNhold(1.0, 0.25, [0.2, 0.1], rng=np.random.default_rng(1))
    Xh, _ = host_span(golden_arm(golden), sim["t"].ravel(), sim["u"], (0.2, 0.1), rule="floor", Ts=0.05)
    assert np.abs(sim["x"] - Xh).max() <= 2e-9
