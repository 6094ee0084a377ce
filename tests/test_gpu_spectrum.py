"""Ksysid.spectrum, spectrum_predict and candidate_spectra on the device: small models fitted to the synthetic pairs of
conftest.synth_pairs (linear and bilinear, poly-2, 300 pairs), the eigenvalues of a matrix logarithm, and the arm golden.
The yardstick is numpy.linalg.eig (LAPACK) of the same matrix, with the bounds of tests/test_gpu_eig.py."""
import numpy as np
import pytest

import _eig_reference as R
import koopman_realizations_amd as kra
from conftest import synth_pairs
from koopman_realizations_amd import _ffi as F

pytestmark = pytest.mark.gpu

EPS = R.EPS
NZ, M = 3, 1


def small_ks(ctx, model_type, **kw):
    """A Ksysid object whose dictionary comes from the constructor (a short made-up trial: it only fixes the sizes and the
    scaling, which the spectrum does not see) and whose model is fitted to the synthetic pairs."""
    rng = np.random.default_rng(11)
    T = 40
    trial = {"t": 0.1 * np.arange(T), "y": rng.uniform(-1, 1, (T, NZ)), "u": rng.uniform(-1, 1, (T, M))}
    ks = kra.Ksysid({"train": [trial], "val": [trial]}, ctx=ctx, model_type=model_type, obs_type=["poly"], obs_degree=[2], **kw)
    ks.snapshotPairs = synth_pairs(300, NZ, M, seed=21)
    return ks.train_models()


@pytest.fixture(scope="module", params=["linear", "bilinear"])
def fitted(request, ctx):
    ks = small_ks(ctx, request.param)
    return ks, ks.spectrum()


def match(a, b):
    d = np.abs(a[:, None] - b[None, :])
    return max(d.min(axis=1).max(), d.min(axis=0).max())


def test_spectrum_matches_lapack(fitted):
    ks, spec = fitted
    A = np.asarray(ks.model["A"])
    N = A.shape[0]
    assert N == ks.params["N"] == 10 and spec["lam"].shape == (N,) and spec["V"].shape == (N, N)
    lam, V = np.linalg.eig(A)
    d, tol = match(spec["lam"], lam), 16 * np.linalg.cond(V) * N * EPS * np.linalg.norm(A)
    r, r_l = R.residual(A, spec["lam"], spec["V"]), R.residual(A, lam, V)
    print(f"{ks.model_type}: eigenvalue distance {d:.3e} (bound {tol:.3e}), r_dev {r:.3f} r_lapack {r_l:.3f}")
    assert d <= tol and r <= max(8 * r_l, 2.0)
    assert np.all(np.diff(np.abs(spec["lam"])) <= 0)
    assert abs(spec["radius"] - np.abs(lam).max()) <= tol
    assert spec["stable"] == bool(spec["radius"] <= 1 + 1e-9)
    assert np.abs(spec["W"] @ spec["V"] - np.eye(N)).max() <= 64 * N * EPS * spec["cond_V"]
    assert np.array_equal(spec["modes"], np.asarray(ks.model["C"]) @ spec["V"])
    assert ks.ctx.timer(F.TIMER_EIG_REGIME) == 1


def test_spectrum_predict_matches_the_host_recursion(fitted):
    ks, spec = fitted
    A, C = np.asarray(ks.model["A"]), np.asarray(ks.model["C"])
    zeta0 = np.array([0.4, -0.3, 0.2])
    z = np.asarray(ks.lift.econ_full(zeta0))
    ref, znorm = np.zeros((21, NZ)), 0.0
    for k in range(21):
        ref[k] = C @ z
        znorm = max(znorm, np.linalg.norm(z))
        z = A @ z
    Y = ks.spectrum_predict(zeta0, 20, spec)
    tol = spec["cond_V"] * 64 * A.shape[0] * EPS * znorm
    print(f"{ks.model_type}: prediction error {np.abs(Y - ref).max():.3e} (bound {tol:.3e}), cond_V {spec['cond_V']:.2e}")
    assert Y.shape == ref.shape and np.abs(Y - ref).max() <= tol
    phi = ks.eigenfunctions(zeta0, spec)
    assert np.abs(phi - spec["W"] @ np.asarray(ks.lift.econ_full(zeta0))).max() == 0


def test_candidate_spectra_of_a_lasso_grid_equals_single_calls(ctx):
    ks = small_ks(ctx, "bilinear", lasso=[0.05, 0.5, 50.0])
    assert len(ks.candidates) == 3
    cs = ks.candidate_spectra()
    assert cs["lam"].shape == (3, 10) and np.array_equal(cs["lasso"], [0.05, 0.5, 50.0])
    for i, c in enumerate(ks.candidates):
        one = ks.spectrum(c, vectors=False)
        assert np.array_equal(cs["lam"][i], one["lam"]) and cs["radius"][i] == one["radius"] and cs["stable"][i] == one["stable"]
    assert np.abs(cs["lam"][0] - cs["lam"][2]).max() > 1e-6          # the grid does give different models
    tab = ks.val_candidates()
    keys = set(tab)
    best, out = ks.select_model("euclid_mean", tab, require_stable=True)
    ok = [i for i in range(3) if cs["stable"][i] and not tab["diverged"][i].any()]
    assert best in ok and set(out) == keys


def test_spectrum_of_the_matrix_logarithm(ctx):
    """eig(logm(K) / Ts) = log(eig(K)) / Ts for a well-conditioned K with its spectrum in the right half of the unit disc, to
    kappa(V) 1e-8: the 1e-8 is kp_logm's square-back tolerance."""
    rng = np.random.default_rng(2)
    lam = np.array([0.9, 0.7, 0.5 + 0.3j, 0.5 - 0.3j, 0.8 + 0.1j, 0.8 - 0.1j])
    D = np.zeros((6, 6))
    D[0, 0], D[1, 1] = 0.9, 0.7
    D[2:4, 2:4] = [[0.5, 0.3], [-0.3, 0.5]]
    D[4:6, 4:6] = [[0.8, 0.1], [-0.1, 0.8]]
    S = np.eye(6) + 0.2 * rng.standard_normal((6, 6))
    K = S @ D @ np.linalg.inv(S)
    Ts = 0.1
    L, nsq, st = ctx.logm(K, 0.0, 1.0 / Ts)
    assert st == F.KP_OK
    lamK, VK, _, stK = ctx.eig(K)
    lamL, _, _, stL = ctx.eig(L, vectors=False)
    assert stK == F.KP_OK and stL == F.KP_OK
    kappa = np.linalg.cond(np.linalg.eig(K)[1])
    assert match(lamK, lam) <= 16 * kappa * 6 * EPS * np.linalg.norm(K)
    d = match(lamL, np.log(lamK) / Ts)
    print(f"eig(logm K / Ts) against log(eig K) / Ts: {d:.3e} (bound {kappa * 1e-8:.3e})")
    assert d <= kappa * 1e-8
    assert match(lamL, np.log(lam) / Ts) <= kappa * 1e-8


def test_arm_model_has_the_constant_observable_and_is_stable(ctx, golden):
    """The linear poly-3 dim_red arm model (the dictionary of test_ct_host.py): the constant observable is carried
    unchanged, an eigenvalue 1 to 1e-9, and the model is reported stable."""
    from _ct_reference import arm_trials
    train, val = arm_trials(golden)
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[3], dim_red=True)
    ks.train_models()
    spec = ks.spectrum()
    A = np.asarray(ks.model["A"])
    lam, V = np.linalg.eig(A)
    N = A.shape[0]
    print(f"arm: N {N} radius {spec['radius']:.12f} |lam - 1| min {np.abs(spec['lam'] - 1).min():.3e} cond_V {spec['cond_V']:.2e}")
    assert match(spec["lam"], lam) <= 16 * np.linalg.cond(V) * N * EPS * np.linalg.norm(A)
    assert np.abs(spec["lam"] - 1.0).min() <= 1e-9
    assert spec["stable"] is True


def test_cli_spectrum_prints_every_candidate_and_stores_the_chosen_eigenvalues(tmp_path):
    import subprocess
    import sys
    from tests._loaded_system import make_trials
    from tests.test_matio import ROOT, write_mat
    f, out = str(tmp_path / "d.mat"), str(tmp_path / "model.npz")
    write_mat(f, make_trials(8, 120, nw=1))
    r = subprocess.run([sys.executable, "-m", "koopman_realizations_amd", "sysid", f, "--model_type", "bilinear", "--obs_degree", "2",
                        "--lasso", "0.05", "50", "--spectrum", "--out", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("spectrum of candidate")]
    assert len(lines) == 2 and all("radius" in ln and "stable" in ln and ln.count("j") == 5 for ln in lines)
    m = np.load(out)
    N = m["A"].shape[0]
    assert m["lam"].shape == (N,) and np.iscomplexobj(m["lam"])
    ref = np.linalg.eigvals(m["A"])
    assert match(m["lam"], ref) <= 16 * np.linalg.cond(np.linalg.eig(m["A"])[1]) * N * EPS * np.linalg.norm(m["A"])


def test_cli_spectrum_of_a_loaded_model_is_refused_in_words_and_the_model_is_still_written(tmp_path):
    import subprocess
    import sys
    from tests._loaded_system import make_trials
    from tests.test_matio import ROOT, write_mat
    f, out = str(tmp_path / "d.mat"), str(tmp_path / "model.npz")
    write_mat(f, make_trials(8, 120, nw=1))
    r = subprocess.run([sys.executable, "-m", "koopman_realizations_amd", "sysid", f, "--model_type", "bilinear", "--obs_degree", "2",
                        "--loaded", "--spectrum", "--out", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--spectrum: not available" in r.stdout and "spectrum of candidate" not in r.stdout
    m = np.load(out)
    assert m["A"].shape == (12, 12) and "lam" not in m.files
