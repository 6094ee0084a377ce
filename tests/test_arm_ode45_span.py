"""arm.ode45_span, the host yardstick of the device arm plant (kp_arm_simulate), against the stored training trials:
they were produced by ONE ode45 call over the whole time vector with outputs from its interpolant and the input row
chosen by Arm.get_k (Arm.m:1004), not by per-sample restarts.  CPU only."""
import numpy as np
import pytest

from _arm_span_reference import golden_arm, host_span
from koopman_realizations_amd.arm import ode45_span


@pytest.fixture(scope="module")
def stored(golden):
    g = golden["arm_data"]
    return golden_arm(golden), g["train_t"][:1201, 0], g["train_u"][:1201], golden["arm_plant"]


def test_get_k_rule_reproduces_the_stored_training_states(stored):
    """The first 200 stored states of trial 0 (arm_plant.npz train_x).  The span runs one sample further, so that
    its stretched last step does not fall on a compared sample."""
    arm, t, u, gp = stored
    X, st = host_span(arm, t[:202], u[:202])
    X = X[:200]
    assert np.abs(X[:, :3] - gp["train_x"][:, :3]).max() <= 1e-10
    assert np.abs(X - gp["train_x"]).max() <= 1e-7
    assert np.abs(arm.get_y(X) - gp["train_y"]).max() <= 1e-10
    assert st["naccept"] > 10000 and st["nreject"] > 0


def test_floor_rule_does_not(stored):
    """simulate_rampNhold's floor(t / Ts) row on the same inputs leaves the stored data within a few samples:
    the stored trials pin the get_k convention."""
    arm, t, u, gp = stored
    X, _ = host_span(arm, t[:32], u[:32], rule="floor", Ts=0.05)
    assert np.abs(X[:30, :3] - gp["train_x"][:30, :3]).max() > 1e-3


def test_ode45_span_outputs_and_arguments():
    """Linear test equation: step ends and interpolated outputs both within the tolerance of the exact solution;
    the first row is y0; argument errors."""
    lam = -2.0
    t = np.linspace(0.0, 3.0, 31)
    st = {}
    Y = ode45_span(lambda s, y: lam * y, t, np.array([1.0, -2.0]), rtol=1e-8, atol=1e-10, stats=st)
    exact = np.exp(lam * t)[:, None] * np.array([1.0, -2.0])
    assert (Y[0] == [1.0, -2.0]).all()
    assert np.abs(Y - exact).max() < 1e-7
    assert st["naccept"] > 0
    with pytest.raises(ValueError):
        ode45_span(lambda s, y: y, [0.0], np.ones(1))
    with pytest.raises(ValueError):
        ode45_span(lambda s, y: y, [0.0, 1.0, 1.0], np.ones(1))


def test_library_exports_kp_arm_simulate():
    from koopman_realizations_amd import _ffi as F
    assert "kp_arm_simulate" in F.ARM_SIGNATURES
    lib = F.lib()
    assert lib.kp_arm_simulate.argtypes is not None


def test_device_arm_output_map_equals_arm_get_y(golden):
    """DeviceArm.get_y is vectorised over rows; its values are Arm.get_y's, bit for bit (no device needed)."""
    import koopman_realizations_amd as kra
    gp = golden["arm_plant"]
    rng = np.random.default_rng(3)
    X = np.vstack([gp["bilin_X"], rng.uniform(-3, 3, (50, 6))])
    for ot in ("markers", "endeff", "angles"):
        a = golden_arm(golden); a.output_type = ot
        d = golden_arm(golden, kra.DeviceArm); d.output_type = ot
        assert np.array_equal(d.get_y(X), a.get_y(X)), ot
        assert np.array_equal(d.get_y(X[4]), a.get_y(X[4])), ot
    p = dict(golden_arm(golden).params); p.update(Nmods=2, nlinks=3, Nlinks=6, nx=12)
    a, d = kra.Arm(p, "markers"), kra.DeviceArm(p, "markers")
    X = rng.uniform(-2, 2, (20, 12))
    assert np.array_equal(d.get_y(X), a.get_y(X))
    with pytest.raises(ValueError):
        d.get_y(np.zeros((2, 5)))
    with pytest.raises(ValueError):
        kra.DeviceArm(dict(p, Nlinks=5), "markers")
