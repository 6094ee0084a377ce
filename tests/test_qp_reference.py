"""The high-precision QP reference (tests/_qp_reference.py) checked on its own, without a GPU: it agrees with the float64
oracle where the oracle is reliable, it moves a wrong candidate active set to the optimum, it tells the optimum from a
point moved off it, and it certifies the degenerate vertices of the stored arm runs (more rows tight than variables, the
pinned first input as a pair of opposite rows), also when H and f are perturbed at the rounding level."""
import numpy as np
import pytest

import _qp_reference as qr
from oracle import koopman_oracle as ko

EPS = np.finfo(np.float64).eps


def _random_qp(rng, n, mr):
    """The shapes of the oracle's own QP test: a tight first row, duplicated rows, an anti-parallel pair pinning row 0 and a
    zero row."""
    M = rng.standard_normal((n, n)); H = M @ M.T + 0.1 * np.eye(n); f = rng.standard_normal(n) * 3
    A = rng.standard_normal((mr, n)); x0 = rng.standard_normal(n); b = A @ x0 + rng.random(mr) * 0.5
    b[0] = A[0] @ x0
    A = np.vstack([A, A[:2], -A[:1], np.zeros((1, n))]); b = np.concatenate([b, b[:2], -b[:1], [0.0]])
    return H, f, A, b


def test_agrees_with_the_oracle_on_random_problems():
    """40 problems, n 2..40: x* equals the oracle's x to 1e3 eps kappa (measured: <= 2e-13 with kappa <= 2e3), and the
    certificate needed no correction of the oracle's active set."""
    rng = np.random.default_rng(7)
    for trial in range(40):
        n = int(rng.integers(2, 41)); mr = int(rng.integers(1, 120))
        H, f, A, b = _random_qp(rng, n, mr)
        xo, lam, ok = ko.qp_solve(H, f, A, b)
        assert ok
        c = qr.certify(H, f, A, b, qr.oracle_active(lam))
        assert c.corrections == 0, trial
        assert np.abs(c.x - xo).max() <= qr.x_error_bound(c, 1e3), (trial, np.abs(c.x - xo).max(), c.kappa)
        # the multipliers certify the KKT conditions in float64 as well
        assert ko.qp_kkt_residual(H, f, A, b, c.x, c.lam) < 1e-10 * (1 + np.abs(f).max())


def test_wrong_start_is_corrected_to_the_same_optimum():
    """From the oracle's set with its last row removed and with a slack row forced in, the corrections reach the optimum the
    oracle's set gives (to the last bits of its float64 rounding)."""
    rng = np.random.default_rng(8)
    for trial in range(12):
        n = int(rng.integers(2, 12)); mr = int(rng.integers(4, 30))
        H, f, A, b = _random_qp(rng, n, mr)
        xo, lam, ok = ko.qp_solve(H, f, A, b)
        act = qr.oracle_active(lam)
        c = qr.certify(H, f, A, b, act)
        starts = [act[:-1]] if act else []
        slack = [int(i) for i in np.nonzero(A @ xo - b < -1e-3)[0]]
        if slack and len(act) < n:
            starts.append(act + slack[:1])
        for st in starts:
            c2 = qr.certify(H, f, A, b, st)
            assert np.abs(c2.x - c.x).max() <= 4 * EPS * max(1.0, np.abs(c.x).max()), (trial, st)
            if set(st) != set(act):
                assert c2.corrections > 0


def test_a_point_moved_off_the_optimum_is_rejected():
    rng = np.random.default_rng(9)
    H, f, A, b = _random_qp(rng, 8, 20)
    xo, lam, ok = ko.qp_solve(H, f, A, b)
    c = qr.certify(H, f, A, b, qr.oracle_active(lam))
    assert qr.check_point(H, f, A, b, c.x, 1e-15, c.active)
    for i in range(8):
        x = c.x.copy(); x[i] += 1e-12 * max(1.0, np.abs(c.x).max())
        assert not qr.check_point(H, f, A, b, x, 1e-15, c.active), i
    # a vertex of the wrong set is not certified as it stands: the certificate corrects it and lands elsewhere
    Hs, fs = np.eye(2), np.array([-2.0, -2.0])
    As, bs = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]), np.array([1.0, 1.0, 1.5])
    c = qr.certify(Hs, fs, As, bs, [0, 1])             # vertex (1, 1) violates row 2
    assert c.corrections > 0 and np.abs(c.x - 0.75).max() < 1e-15 and c.active == [2]


def test_infeasible_problems_are_not_certified():
    with pytest.raises(qr.NotCertified):
        qr.certify(np.eye(2), np.zeros(2), np.array([[1.0, 0], [-1.0, 0]]), np.array([-1.0, -1.0]))
    with pytest.raises(qr.NotCertified):
        qr.certify(np.eye(2), np.zeros(2), np.zeros((1, 2)), np.array([-1e-3]))


@pytest.fixture(scope="module")
def stored_run_qps(arm, golden):
    """The QPs of every 15th step of the stored bilinear and linear block-M runs (teacher-forced, as
    tools/qp_robustness_probe.py takes them), assembled by the oracle."""
    r = golden["arm_blockM"]; sc = arm["scale"]
    ysc = (golden["blockM_ref"]["y"] - sc["y_offset"][-2:]) / sc["y_factor"][-2:]
    out = []
    for mt, key in (("bilinear", "bilin"), ("linear", "lin")):
        # example_sysid.m / example_control.m settings of the stored runs: poly-3 with dim_red, horizon 10, slope 0.1,
        # costs 10 / 100 / 0.1 [3e-2, 2e-2, 1e-2], no input box, projection on the end effector
        dic = ko.build_dictionary(mt, 6, 3, ["poly"], [3], arm["pairs"], dim_red=True)
        koop = ko.get_koopman(dic, arm["pairs"])
        mdl = ko.get_blmodel(dic, koop, 6) if mt == "bilinear" else ko.get_model(dic, koop, 6)
        s = ko.MpcSetup(model_type=mt, A=mdl["A"], B=mdl["B"], m=3, Np=10, projmtx=mdl["C"][-2:, :], cost_running=10.0,
                        cost_terminal=100.0, cost_input=0.1 * np.array([3e-2, 2e-2, 1e-2]), input_bounds=None,
                        slope_lim=1e-1 * sc["u_factor"].mean(), smooth_lim=None, n=6)
        Y, U = r[key + "_Y"], r[key + "_U"]
        for k in range(0, 299, 15):
            z = ko.econ_full(dic, ko.scaledown(sc, "y", Y[k])[None, :])[0]
            out.append((mt, k) + tuple(ko.mpc_qp(s, z, ko.scaledown(sc, "u", U[k]), ysc[k:k + 11])))
    return out


def test_certifies_the_degenerate_vertices_of_the_stored_runs(stored_run_qps):
    """The stored runs' QPs (30 variables, slope rows and the pinned first input: rows 3..5 tight twice over) sit at
    primal-degenerate vertices: more rows tight than variables on many steps.  The reference certifies each one, from the
    oracle's set and from that set with its last row removed, the oracle agrees to 1e3 eps kappa, and when H and f are
    perturbed at 1e-10 relative (another rounding of the assembly) the certified optimum moves by no more than the
    perturbation allows (the float64 oracle may or may not survive those; the reference must)."""
    rng = np.random.default_rng(10)
    degenerate = 0
    for mt, k, H, f, A, b in stored_run_qps:
        xo, lam, ok = ko.qp_solve(H, f, A, b)
        assert ok, (mt, k)
        act = qr.oracle_active(lam)
        c = qr.certify(H, f, A, b, act)
        tight = int((np.abs(A @ c.x - b) <= 1e-12 * (1 + np.abs(b))).sum())
        degenerate += tight > H.shape[0]
        assert np.abs(c.x - xo).max() <= qr.x_error_bound(c, 1e3), (mt, k, np.abs(c.x - xo).max(), c.kappa)
        if act:
            c2 = qr.certify(H, f, A, b, act[:-1])
            assert np.abs(c2.x - c.x).max() <= 8 * EPS * max(1.0, np.abs(c.x).max()), (mt, k)
        E = 1e-10 * rng.standard_normal(H.shape) * np.sqrt(np.outer(np.diag(H), np.diag(H)))
        Hp, fp = H + 0.5 * (E + E.T), f * (1 + 1e-10 * rng.standard_normal(f.shape))
        xp, lamp, okp = ko.qp_solve(Hp, fp, A, b)
        cp = qr.certify(Hp, fp, A, b, qr.oracle_active(lamp) if okp else act)
        assert np.abs(cp.x - c.x).max() <= 1e-10 * c.kappa * max(1.0, np.abs(c.x).max()) * 100, (mt, k)
        if okp:
            assert np.abs(xp - cp.x).max() <= qr.x_error_bound(cp, 1e3), (mt, k)
    assert degenerate >= 8, degenerate                  # measured: 11 of the 40 sampled steps
