"""Ksysid.spectrum, eigenfunctions, spectrum_predict, candidate_spectra and select_model(require_stable) without a device:
objects built without the constructor, ctx.eig replaced by the numpy restatement of the kernel (tests/_eig_reference.py)
behind the same unpacking and sorting that Context.eig applies."""
import numpy as np
import pytest

import _eig_reference as R
from koopman_realizations_amd import _ffi as F
from koopman_realizations_amd.device import eig_unpack
from koopman_realizations_amd.ksysid import Ksysid


class FakeCtx:
    """Context.eig with the restatement in place of kp_eig."""
    calls = 0

    def eig(self, A, vectors=True):
        self.calls += 1
        A = np.asarray(A, dtype=np.float64)
        single = A.ndim == 2
        wr, wi, Vp, it, st = R.eig_batch(A[None] if single else A, vectors)
        lam, V = eig_unpack(wr, wi, Vp)
        if single:
            return lam[0], (None if V is None else V[0]), int(it[0]), int(st[0])
        return lam, V, it, st


class IdentityLift:
    """psi(zeta) = zeta: the lifted state of a linear dictionary of degree 1 without the constant."""
    @staticmethod
    def econ_full(v):
        return np.asarray(v, dtype=np.float64)


def _bare(A, time_type="discrete", model_type="linear", n=2, Ts=0.1):
    ks = Ksysid.__new__(Ksysid)
    N = A.shape[0]
    ks.ctx, ks.lift = FakeCtx(), IdentityLift()
    ks.params = {"n": n, "m": 1, "N": N, "Ts": Ts, "nd": 0, "nw": 0}
    ks.loaded, ks.model_type, ks.time_type = False, model_type, time_type
    ks.model = {"A": A, "B": np.zeros((N, 1)), "C": np.hstack([np.eye(n), np.zeros((n, N - n))])}
    ks.candidates = ks.model
    return ks


def _stable_matrix(N=7, seed=5):
    return R.random_matrix("stable", N, seed)


def test_sorting_and_the_pair_order():
    ks = _bare(_stable_matrix())
    spec = ks.spectrum()
    lam = spec["lam"]
    assert lam.dtype == complex and np.all(np.diff(np.abs(lam)) <= 0)
    ref = np.linalg.eigvals(ks.model["A"])
    assert np.abs(np.sort_complex(lam) - np.sort_complex(ref)).max() < 1e-13
    j = 0
    while j < len(lam):
        if lam[j].imag != 0:
            assert lam[j].imag > 0 and lam[j + 1] == np.conj(lam[j])
            j += 2
        else:
            j += 1
    assert spec["radius"] == np.abs(lam).max() and abs(spec["radius"] - 0.8) < 1e-12
    # equal moduli (a cyclic shift: the whole spectrum on the unit circle) keep every pair together
    lam = _bare(R.cyclic(7)).spectrum(vectors=False)["lam"]
    pairs = [j for j in range(7) if lam[j].imag > 0]
    assert len(pairs) == 3 and all(lam[j + 1] == np.conj(lam[j]) for j in pairs)


def test_exponent_and_stable_of_a_discrete_model():
    ks = _bare(np.diag([1.0 + 1e-12, 0.5, -0.25]), Ts=0.1)
    spec = ks.spectrum()
    assert np.array_equal(spec["lam"], [1.0 + 1e-12, 0.5, -0.25])
    assert spec["stable"] is True                      # 1 + 1e-12: the constant observable to rounding
    assert np.allclose(spec["exponent"], np.log(spec["lam"].astype(complex)) / 0.1, rtol=0, atol=1e-13)
    assert np.allclose(spec["decay"], [1e-11, np.log(0.5) / 0.1, np.log(0.25) / 0.1], rtol=0, atol=1e-9)
    assert np.allclose(spec["freq_hz"], [0.0, 0.0, np.pi / 0.1 / (2 * np.pi)])
    assert _bare(np.diag([1.0 + 1e-6, 0.5])).spectrum()["stable"] is False
    assert _bare(np.diag([1.0 + 1e-6, 0.5])).spectrum(stable_tol=1e-5)["stable"] is True
    assert _bare(np.zeros((3, 3))).spectrum(vectors=False)["stable"] is True          # log 0 = -inf, quietly


def test_exponent_and_stable_of_a_continuous_model():
    A = np.array([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.0], [0.0, 0.0, 1e-12]])            # the generator: rates and frequencies
    spec = _bare(A, "continuous").spectrum()
    assert np.array_equal(spec["exponent"], spec["lam"])
    assert spec["stable"] is True and np.allclose(sorted(spec["decay"]), [-0.5, -0.5, 1e-12])
    assert np.allclose(sorted(spec["freq_hz"]), [0.0, 2.0 / (2 * np.pi), 2.0 / (2 * np.pi)])
    A[2, 2] = 1e-3
    assert _bare(A, "continuous").spectrum()["stable"] is False
    assert _bare(10.0 * A - 20.0 * np.eye(3), "continuous").spectrum()["stable"] is True          # radius > 1 does not matter


def test_left_eigenvectors_and_modes():
    ks = _bare(_stable_matrix())
    spec = ks.spectrum()
    N = 7
    assert np.abs(spec["W"] @ spec["V"] - np.eye(N)).max() < 1e-12
    assert np.abs(spec["W"] @ ks.model["A"] - spec["lam"][:, None] * spec["W"]).max() < 1e-12      # rows: left eigenvectors
    assert np.array_equal(spec["modes"], ks.model["C"] @ spec["V"]) and spec["modes"].shape == (2, N)
    assert abs(spec["cond_V"] - np.linalg.cond(spec["V"])) < 1e-9 * spec["cond_V"]
    no = ks.spectrum(vectors=False)
    assert not {"V", "W", "modes", "cond_V"} & set(no) and np.allclose(no["lam"], spec["lam"], rtol=0, atol=1e-13)


def test_eigenfunctions_advance_by_their_eigenvalue():
    ks = _bare(_stable_matrix())
    spec = ks.spectrum()
    A = ks.model["A"]
    rng = np.random.default_rng(0)
    z = rng.uniform(-1, 1, 7)
    assert np.abs(ks.eigenfunctions(A @ z, spec) - spec["lam"] * ks.eigenfunctions(z, spec)).max() < 1e-12
    Zr = rng.uniform(-1, 1, (4, 7))
    rows = ks.eigenfunctions(Zr, spec)
    assert rows.shape == (4, 7) and np.abs(rows[2] - ks.eigenfunctions(Zr[2], spec)).max() < 1e-14
    assert np.abs(ks.eigenfunctions(Zr @ A.T, spec) - rows * spec["lam"][None, :]).max() < 1e-12


@pytest.mark.parametrize("model_type", ["linear", "bilinear"])
def test_spectrum_predict_equals_the_recursion(model_type):
    ks = _bare(_stable_matrix(), model_type=model_type)
    spec = ks.spectrum()
    A, C = ks.model["A"], ks.model["C"]
    z = np.random.default_rng(1).uniform(-1, 1, 7)
    Y = ks.spectrum_predict(z, 20, spec)
    ref = np.zeros((21, 2))
    zk = z.copy()
    for k in range(21):
        ref[k] = C @ zk
        zk = A @ zk
    assert Y.shape == (21, 2) and Y.dtype == np.float64
    assert np.abs(Y - ref).max() <= spec["cond_V"] * 64 * 7 * R.EPS * np.abs(z).max() * np.sqrt(7)


def test_spectrum_predict_of_a_continuous_model_is_the_flow_of_its_generator():
    G = np.array([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.3], [0.0, 0.0, -0.1]])
    ks = _bare(G, "continuous", Ts=0.05)
    spec = ks.spectrum()
    z = np.array([1.0, -0.5, 0.25])
    Y = ks.spectrum_predict(z, 10, spec)
    lam, V = np.linalg.eig(G)                          # LAPACK's flow
    for k in range(11):
        zk = np.real(V @ (np.exp(lam * k * 0.05) * np.linalg.solve(V, z)))
        assert np.abs(Y[k] - zk[:2]).max() < 1e-12


def test_refusals():
    A = _stable_matrix()
    ks = _bare(A, model_type="nonlinear")
    ks.model = {"Kf": np.zeros((2, 9)), "C": np.eye(2)}
    with pytest.raises(ValueError, match="square operator"):
        ks.spectrum()
    ks = _bare(A)
    ks.loaded = True
    with pytest.raises(NotImplementedError):
        ks.spectrum()
    with pytest.raises(NotImplementedError):
        ks.candidate_spectra()
    ks = _bare(np.zeros((F.EIG_MAXN + 1, F.EIG_MAXN + 1)))
    with pytest.raises(ValueError, match="512"):
        ks.spectrum()
    assert ks.ctx.calls == 0
    ks = _bare(A)
    ks.model = None
    with pytest.raises(ValueError, match="train_models"):
        ks.spectrum()
    bad = A.copy()
    bad[0, 0] = np.nan
    with pytest.raises(F.KoopmanHipError):
        _bare(bad).spectrum()


def _candidates():
    S = _stable_matrix()
    mats = [S, 1.5 * S, 0.5 * S]                       # radius 0.8, 1.2, 0.4
    ks = _bare(S)
    ks.candidates = [dict(ks.model, A=M, lasso=float(10 ** i)) for i, M in enumerate(mats)]
    ks.model = ks.candidates[0]
    return ks


def test_candidate_spectra_is_one_call_for_all_candidates():
    ks = _candidates()
    cs = ks.candidate_spectra()
    assert ks.ctx.calls == 1
    assert cs["lam"].shape == (3, 7) and np.allclose(cs["radius"], [0.8, 1.2, 0.4], rtol=0, atol=1e-12)
    assert list(cs["stable"]) == [True, False, True] and list(cs["lasso"]) == [1.0, 10.0, 100.0]
    for i, c in enumerate(ks.candidates):
        assert np.array_equal(cs["lam"][i], ks.spectrum(c, vectors=False)["lam"])
    assert "lasso" not in ks.candidate_spectra([{"A": c["A"], "C": c["C"]} for c in ks.candidates])
    bad = ks.candidates[0]["A"].copy()
    bad[1, 1] = np.inf
    cs = ks.candidate_spectra([dict(ks.candidates[0], A=bad), ks.candidates[2]])
    assert list(cs["stable"]) == [False, True] and np.all(np.isnan(cs["lam"][0]))


def _table(euclid, diverged=None, n=2):
    euclid = np.asarray(euclid, dtype=np.float64)
    nmod, ntr = euclid.shape
    per_out = np.repeat(euclid[:, :, None], n, axis=2)
    return {"mean": per_out.copy(), "rmse": per_out.copy(), "nrmse": per_out.copy(), "euclid_mean": euclid,
            "unscaled_euclid_mean": 3.0 * euclid,
            "diverged": np.zeros((nmod, ntr), dtype=bool) if diverged is None else np.asarray(diverged, dtype=bool)}


def test_select_model_require_stable_ranks_unstable_candidates_last():
    ks = _candidates()
    tab = _table([[0.3, 0.5], [0.1, 0.2], [0.35, 0.6]])          # the unstable candidate 1 validates best
    keys = set(tab)
    best, out = ks.select_model(table=tab)                        # the default: as before, and no eigensolver call
    assert best == 1 and out is tab and ks.model is ks.candidates[1] and ks.ctx.calls == 0
    best, out = ks.select_model(table=tab, require_stable=True)
    assert best == 0 and ks.model is ks.candidates[0] and ks.ctx.calls == 1 and set(out) == keys
    tab["stable"] = np.array([False, True, True])                 # a hand-made column is taken as it stands
    assert ks.select_model(table=tab, require_stable=True)[0] == 1 and ks.ctx.calls == 1
    assert ks.select_model(table=tab)[0] == 1
    tab["stable"] = np.array([True, True, True])
    tab["diverged"][1, 0] = True
    assert ks.select_model(table=tab, require_stable=True)[0] == 0
    tab["stable"] = np.array([False, True, False])
    before = ks.model
    with pytest.raises(ValueError, match="unstable"):
        ks.select_model(table=tab, require_stable=True)
    assert ks.model is before
