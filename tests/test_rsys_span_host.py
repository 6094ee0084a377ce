"""Rsys.simulate_systems_ode45: the reference's own integration of the random systems (Rsys.m:118: ONE ode45 call over
tq per trial, inputs by get_u, outputs from ode45's interpolant), the host yardstick of the device span mode."""
import numpy as np

from koopman_realizations_amd.rsys import Rsys


def test_layout_accuracy_and_step_count():
    """The shipped layout (1 001 rows, t from 0 to 10) and the same draws as simulate_systems, with at least 20x fewer
    steps than its per-sample restarts.  One span over inputs that jump every 50 samples is as accurate as ode45 makes it:
    its error estimate does not see the jumps, so at the default RelTol 1e-3 a trial is off by up to a few 1e-1 here (not
    a defect of the restatement); it converges to the restarts as the tolerance tightens (2e-3 at 1e-5, 1e-8 at 1e-11)."""
    from koopman_realizations_amd.arm import dopri45
    x0 = np.zeros((1, 1))
    r = Rsys(1, 3, 3, 2, seed=5)
    got = r.simulate_systems_ode45(10.0, 0.01, 2, x0)
    steps = r.last_stats["naccept"] + r.last_stats["nreject"]
    ref = Rsys(1, 3, 3, 2, seed=5).simulate_systems(10.0, 0.01, 2, x0)
    finer = Rsys(1, 3, 3, 2, seed=5).simulate_systems_ode45(10.0, 0.01, 2, x0, rtol=1e-5, atol=1e-8)
    tight = Rsys(1, 3, 3, 2, seed=5).simulate_systems_ode45(10.0, 0.01, 2, x0, rtol=1e-11, atol=1e-13)
    for j in range(2):
        g, w = got[j][0], ref[j][0]
        assert g["y"].shape == (1001, 1) and g["u"].shape == (1001, 1)
        assert g["t"][0] == 0.0 and abs(g["t"][-1] - 10.0) < 1e-12 and np.array_equal(g["t"], w["t"])
        assert np.array_equal(g["u"], w["u"])
        assert g["y"][0, 0] == 0.0 and np.isfinite(g["y"]).all()
        assert np.abs(g["y"] - w["y"]).max() <= 0.5
        assert np.abs(finer[j][0]["y"] - w["y"]).max() <= 2e-3
        assert np.abs(tight[j][0]["y"] - w["y"]).max() <= 1e-8
    # the restarts' step count (Rsys.simulate_systems' dopri45 from sample to sample), first trial
    f = r.systems[0]["vf_func"]
    tq, uq, y, st = ref[0][0]["t"], ref[0][0]["u"][:, 0], np.zeros(1), {}
    for k in range(len(tq) - 1):
        uk = uq[k]
        y = dopri45(lambda t, x: f(t, x, uk), tq[k], tq[k + 1], y, stats=st)
    assert steps[0, 0] * 20 <= st["naccept"] + st.get("nreject", 0), (steps[0, 0], st)


def test_get_u_rows_at_sample_boundaries():
    """get_u (Rsys.m:128-133): the last sample at or before t - so a stage that lands exactly on t_k sees row k, one just
    before it row k - 1, and times past the end the last row.  simulate_systems_ode45 selects its inputs this way."""
    tq = np.arange(0.0, 1.0 + 0.005, 0.01)
    uq = np.arange(tq.size, dtype=np.float64)
    for k in (0, 1, 49, 50, 51, 100):
        assert Rsys.get_u(tq[k], tq, uq) == k
        if k:
            assert Rsys.get_u(np.nextafter(tq[k], -np.inf), tq, uq) == k - 1
        if k < 100:
            assert Rsys.get_u(0.5 * (tq[k] + tq[k + 1]), tq, uq) == k
    assert Rsys.get_u(5.0, tq, uq) == 100
    # the integration sees exactly these rows: inputs that are zero except on one sample row leave a trace only if some
    # stage time lands in [t_k, t_{k+1})
    r = Rsys(1, 1, 1, 1, seed=0)
    r.systems[0].update(coeffs=np.zeros(1), pow_x=np.zeros(1, int), pow_u=np.zeros(1, int), input_gain=1.0)
    seen = []
    orig = Rsys.get_u_row

    def spy(t, tq_):
        k = orig(t, tq_)
        seen.append((t, k))
        return k
    try:
        Rsys.get_u_row = staticmethod(spy)
        r.simulate_systems_ode45(1.0, 0.01, 1, np.zeros((1, 1)), inputs=np.zeros((1, 1, tq.size)))
    finally:
        Rsys.get_u_row = staticmethod(orig)
    assert seen
    for t, k in seen:
        assert tq[k] <= t and (k == tq.size - 1 or t < tq[k + 1]), (t, k)
