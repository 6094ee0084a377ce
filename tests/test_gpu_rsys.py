"""The device random-system generator (kp_rsys_simulate, kra.DeviceRsys) against the host mirror
Rsys.simulate_systems_fast / arm.dopri45 (restart mode) and the host yardstick Rsys.simulate_systems_ode45 (span mode,
the reference's one ode45 call per trial), the resident sweep on its Traj, batch independence, per-trial failure and
argument errors.  One GPU lane per (system, trial); see include/koopman_hip_rsys.h for the modes and input forms."""
import ctypes as C

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from koopman_realizations_amd import sweep
from koopman_realizations_amd.arm import dopri45
from koopman_realizations_amd.rsys import Rsys

pytestmark = pytest.mark.gpu

SHAPE = (64, 3, 3, 2)          # the set test_gpu_sweep.py generates: 64 systems, 3 terms, degree_x 3, degree_u 2
X0 = np.zeros((1, 1))


def _arrays(r):
    co = np.stack([s["coeffs"] for s in r.systems]); px = np.stack([s["pow_x"] for s in r.systems])
    pu = np.stack([s["pow_u"] for s in r.systems]); cu = np.array([s["input_gain"] for s in r.systems])
    return co, px, pu, cu


def test_restart_mode_matches_the_host_mirror(ctx):
    """DeviceRsys.simulate_systems_restart = Rsys.simulate_systems_fast on 64 systems x 11 trials x 1001 samples: the
    same draws, inputs identical, |dY| <= 1e-9 everywhere, and each sampled trial's (naccept, nreject) equal to those of
    arm.dopri45 run sample to sample under the held input (Rsys.simulate_systems' integration)."""
    d = kra.DeviceRsys(*SHAPE, seed=21, ctx=ctx)
    got = d.simulate_systems_restart(10.0, 0.01, 11, X0)
    ref = Rsys(*SHAPE, seed=21).simulate_systems_fast(10.0, 0.01, 11, X0)
    worst = 0.0
    for j in range(11):
        for i in range(64):
            assert np.array_equal(got[j][i]["u"], ref[j][i]["u"]), (i, j)
            assert np.array_equal(got[j][i]["t"], ref[j][i]["t"])
            worst = max(worst, np.abs(got[j][i]["y"] - ref[j][i]["y"]).max())
    assert worst <= 1e-9, worst
    assert (d.last_stats["status"] == 0).all()
    tq = got[0][0]["t"]
    for i, j in ((0, 0), (17, 5), (63, 10)):
        f = d.systems[i]["vf_func"]
        uq = ref[j][i]["u"][:, 0]
        y = ref[j][i]["y"][0].copy()
        st = {}
        for k in range(len(tq) - 1):
            uk = uq[k]
            y = dopri45(lambda t, x: f(t, x, uk), tq[k], tq[k + 1], y, stats=st)
        assert (d.last_stats["naccept"][i, j], d.last_stats["nreject"][i, j]) == (st["naccept"], st.get("nreject", 0)), (i, j)


LANES = [(i, j) for i, j in zip(range(0, 64, 4), (0, 3, 7, 10, 1, 5, 9, 2, 6, 8, 4, 10, 0, 7, 3, 9))]     # 16 lanes across systems


def test_span_mode_matches_the_host_ode45_yardstick(ctx):
    """Span mode (Rsys.m:118: ONE ode45 over tq, get_u rows, ntrp45 outputs) against Rsys.simulate_systems_ode45 on 16
    lanes across systems, with the reference's held levels (hold = 50) and with a new input at every sample (hold = 0,
    the shipped sets' form): equal (naccept, nreject) and |dY| <= 1e-8.  The outputs typically agree to 1e-11; the
    last-bit differences of exp / atan / pow and of the summation order grow along a trajectory whose input jumps, to a
    few 1e-9 on the worst of these lanes.  The single span takes under 1/20 of the steps of the per-sample restarts."""
    d = kra.DeviceRsys(*SHAPE, seed=21, ctx=ctx)
    got = d.simulate_systems(10.0, 0.01, 11, X0)
    span_steps = d.last_stats["naccept"] + d.last_stats["nreject"]
    h = Rsys(*SHAPE, seed=21)
    ref = h.simulate_systems_ode45(10.0, 0.01, 11, X0, lanes=LANES)
    for i, j in LANES:
        assert np.array_equal(got[j][i]["u"], ref[j][i]["u"]), (i, j)
        assert np.abs(got[j][i]["y"] - ref[j][i]["y"]).max() <= 1e-8, (i, j)
        assert d.last_stats["naccept"][i, j] == h.last_stats["naccept"][i, j], (i, j)
        assert d.last_stats["nreject"][i, j] == h.last_stats["nreject"][i, j], (i, j)
    d2 = kra.DeviceRsys(*SHAPE, seed=21, ctx=ctx)
    d2.simulate_systems_restart(10.0, 0.01, 11, X0)
    restart_steps = d2.last_stats["naccept"] + d2.last_stats["nreject"]
    assert span_steps.sum() * 20 < restart_steps.sum(), (span_steps.sum(), restart_steps.sum())

    # hold = 0: every row given, a new input at every sample
    r = Rsys(16, 3, 3, 2, seed=5)
    co, px, pu, cu = _arrays(r)
    tq = np.arange(0.0, 10.0 + 0.005, 0.01)
    U = np.random.default_rng(3).uniform(-1, 1, (16, 2, tq.size))
    x0 = np.array([0.0, 0.5])
    Y, na, nr, st = ctx.rsys_simulate("span", tq, co, px, pu, cu, x0, U, hold=0, degree_x=3, degree_u=2)
    assert (st == 0).all()
    lanes = [(i, i % 2) for i in range(16)]
    ref = r.simulate_systems_ode45(10.0, 0.01, 2, x0[:, None], inputs=U, lanes=lanes)
    for i, j in lanes:
        assert np.abs(Y[i, j] - ref[j][i]["y"][:, 0]).max() <= 1e-8, (i, j)
        assert (na[i, j], nr[i, j]) == (r.last_stats["naccept"][i, j], r.last_stats["nreject"][i, j]), (i, j)


def test_resident_sweep_equals_the_uploaded_sweep(ctx):
    """rand_models_sweep_traj on the Traj that simulate_to_traj leaves on the device = rand_models_sweep_batched on
    Rsys.save_data of the Y / U the same call returned to the host (uploaded by kp_traj_create / put / finish), bit for
    bit with NaNs in the same places; the object's layout and device scaling are those of the upload."""
    d = kra.DeviceRsys(*SHAPE, seed=21, ctx=ctx)
    degrees = {"linear": 13, "bilinear": 6, "nonlinear": 4}
    traj = d.simulate_to_traj(10.0, 0.01, 11, X0, keep_host=True)
    try:
        assert (traj.nb, traj.ntrials, traj.T, traj.n, traj.m, traj.Tv) == (64, 10, 1001, 1, 1, 1001)
        tr = d.last_Y[:, :10].reshape(64, -1)
        tu = d.last_U[:, :10].reshape(64, -1)
        sc = traj.scale()
        lo, hi = tr.min(axis=1), tr.max(axis=1)
        assert np.allclose(sc[:, 0], (hi + lo) / 2, rtol=0, atol=1e-15) and np.allclose(sc[:, 1], (hi - lo) / 2, rtol=0, atol=1e-15)
        assert np.allclose(sc[:, 2], (tu.max(axis=1) + tu.min(axis=1)) / 2, rtol=0, atol=1e-15)
        got = sweep.rand_models_sweep_traj(traj, ctx, degrees=degrees)
        assert traj.handle                                   # the caller keeps the object
    finally:
        traj.close()
    U = d.last_U
    systems = Rsys.save_data([[{"t": d.last_t, "y": d.last_Y[i, j][:, None], "u": U[i, j][:, None]} for i in range(64)]
                              for j in range(11)])
    assert sweep._stack_raw(systems) is not None          # the resident path, not the host-prepared fallback
    ref = sweep.rand_models_sweep_batched(systems, ctx, degrees=degrees)
    for mt in degrees:
        assert got[mt].shape == (degrees[mt], 64)
        assert np.array_equal(np.isnan(got[mt]), np.isnan(ref[mt])), mt
        assert np.array_equal(got[mt], ref[mt], equal_nan=True), (mt, np.nanmax(np.abs(got[mt] - ref[mt])))


def test_batch_independence(ctx):
    """A lane run alone is bit-identical to the same lane inside a batch of 65 systems, in both modes and input forms."""
    r = Rsys(65, 3, 3, 2, seed=9)
    co, px, pu, cu = _arrays(r)
    tq = np.arange(0.0, 2.0 + 0.005, 0.01)
    rng = np.random.default_rng(4)
    for hold, U in ((0, rng.uniform(-1, 1, (65, 1, tq.size))), (50, rng.uniform(-1, 1, (65, 1, -(-tq.size // 50))))):
        for mode in ("span", "restart"):
            Y, na, nr, st = ctx.rsys_simulate(mode, tq, co, px, pu, cu, [0.3], U, hold=hold, degree_x=3, degree_u=2)
            assert (st == 0).all()
            for k in (0, 1, 63, 64):
                Y1, na1, nr1, st1 = ctx.rsys_simulate(mode, tq, co[k:k + 1], px[k:k + 1], pu[k:k + 1], cu[k:k + 1], [0.3], U[k:k + 1],
                                                      hold=hold, degree_x=3, degree_u=2)
                assert np.array_equal(Y1[0], Y[k]) and na1[0, 0] == na[k, 0] and nr1[0, 0] == nr[k, 0], (mode, hold, k)


def test_per_trial_failure(ctx):
    """A trial that cannot be integrated fails alone: status KP_ERR_NOT_CONVERGED and NaN rows from its first output on,
    the other trials as in a run without it.  A tolerance the step control cannot meet (rtol = atol = 1e-300) fails every
    trial; with a Traj requested the call reports KP_ERR_NOT_CONVERGED and creates no object."""
    r = Rsys(8, 3, 3, 2, seed=2)
    co, px, pu, cu = _arrays(r)
    tq = np.arange(0.0, 1.0 + 0.005, 0.01)
    U = np.random.default_rng(1).uniform(-1, 1, (8, 3, 3))
    for mode in ("span", "restart"):
        Y, _, _, st, tr = ctx.rsys_simulate(mode, tq, co, px, pu, cu, [0.0, 0.2, 0.4], U, hold=50, degree_x=3, degree_u=2,
                                            rtol=1e-300, atol=1e-300, want_traj=True)
        assert tr is None and (st == F.KP_ERR_NOT_CONVERGED).all(), mode
        assert np.isnan(Y[:, :, 1:]).all() and (Y[:, :, 0] == [0.0, 0.2, 0.4]).all()
        ok = ctx.rsys_simulate(mode, tq, co, px, pu, cu, [0.0, 0.4], U[:, [0, 2]], hold=50, degree_x=3, degree_u=2)[0]
        Y, _, _, st, tr = ctx.rsys_simulate(mode, tq, co, px, pu, cu, [0.0, np.nan, 0.4], U, hold=50, degree_x=3, degree_u=2,
                                            want_traj=True)
        assert tr is None
        assert (st[:, 1] == F.KP_ERR_NOT_CONVERGED).all() and (st[:, [0, 2]] == F.KP_OK).all(), mode
        assert np.isnan(Y[:, 1]).all() and np.array_equal(Y[:, [0, 2]], ok), mode
        with pytest.raises(F.KoopmanHipError) as e:
            F.check(F.lib().kp_rsys_simulate(ctx.handle, C.byref(F.KpRsysDims(3, 3, 2)), 0, 8, 3, tq.size, F.dptr(tq), F.dptr(co),
                                             _ip(px), _ip(pu), F.dptr(cu), F.dptr(np.array([0.0, np.nan, 0.4])), F.dptr(U), 50,
                                             1e-3, 1e-6, None, None, None, _ip(np.zeros((8, 3), np.int32)), C.byref(F.vp())),
                    ctx.handle)
        assert e.value.code == F.KP_ERR_NOT_CONVERGED


def _with(a, v):
    a = np.array(a, dtype=np.int32)
    a[1, 2] = v
    return a


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(F.c_ip)


def test_argument_errors(ctx):
    """Every KP_ERR_ARG case of kp_rsys_simulate, with a message that names the entry point."""
    r = Rsys(2, 3, 3, 2, seed=1)
    co, px, pu, cu = _arrays(r)
    px = np.ascontiguousarray(px, dtype=np.int32); pu = np.ascontiguousarray(pu, dtype=np.int32)
    tq = np.arange(0.0, 0.1 + 0.005, 0.01)
    x0 = np.zeros(2)
    U = np.zeros((2, 2, tq.size))
    keep = []

    def call(dims=(3, 3, 2), mode=0, nsys=2, ntrials=2, T=None, t=tq, coeffs=co, pow_x=px, pow_u=pu, gain=cu, x0=x0, U=U,
             hold=0, rtol=1e-3, atol=1e-6, status=True, traj=False):
        st = np.zeros((2, 2), np.int32)
        Y = np.zeros((2, 2, tq.size))
        h = F.vp()
        keep.append((st, Y))
        d = None if dims is None else C.byref(F.KpRsysDims(*dims))
        return F.lib().kp_rsys_simulate(ctx.handle, d, mode, nsys, ntrials, tq.size if T is None else T, F.dptr(t), F.dptr(coeffs),
                                        _ip(pow_x), _ip(pow_u), F.dptr(gain), F.dptr(x0), F.dptr(U), hold, rtol, atol, F.dptr(Y),
                                        None, None, _ip(st) if status else None, C.byref(h) if traj else None)

    assert call() == F.KP_OK
    bad = [dict(nsys=0), dict(dims=(0, 3, 2)), dict(ntrials=1, traj=True), dict(ntrials=0), dict(T=2),
           dict(dims=(3, 16, 2)), dict(dims=(3, 3, 16)), dict(dims=(3, -1, 2)), dict(dims=(3, 3, -1)),
           dict(pow_x=_with(px, 4)), dict(pow_x=_with(px, -1)), dict(pow_u=_with(pu, 3)), dict(pow_u=_with(pu, -1)),
           dict(t=np.concatenate([[0.01], tq[1:] + 0.01])), dict(t=np.concatenate([tq[:5], tq[4:-1]])),
           dict(t=np.concatenate([tq[:5], [np.nan], tq[6:]])),
           dict(rtol=0.0), dict(rtol=-1e-3), dict(rtol=np.inf), dict(atol=0.0), dict(atol=np.nan),
           dict(mode=2), dict(mode=-1), dict(hold=-1), dict(dims=None), dict(t=None), dict(coeffs=None), dict(pow_x=None),
           dict(pow_u=None), dict(gain=None), dict(x0=None), dict(U=None), dict(status=False)]
    for kw in bad:
        assert call(**kw) == F.KP_ERR_ARG, kw
        assert F.lib().kp_last_error(ctx.handle).decode().startswith("kp_rsys_simulate"), kw
    with pytest.raises(ValueError):
        ctx.rsys_simulate("span", tq, co, px, pu, cu, x0, U[:, :, :5], hold=0)
