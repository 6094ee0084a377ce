"""The numpy restatement of kp_eig (tests/_eig_reference.py) against numpy.linalg.eig on the case list of the GPU test
(tests/test_gpu_eig.py), with its bounds: the residual r <= max(8 r_lapack, 2), every eigenvalue within
16 kappa_2(V_lapack) n eps ||A||_F of a LAPACK eigenvalue in both directions, the two power sums, pairs adjacent with the
positive imaginary part first, and the balancing case to 1e-12 radius.  The sizes are those of the device test: both sides of
the wave limit and of the header's two LDS limits, 257 with vectors, 512 with values only, once."""
import math

import numpy as np
import pytest

import _eig_reference as R
from koopman_realizations_amd import _ffi as F

EPS = R.EPS
L_VEC, L_VAL = F.EIG_LDS_MAXN_VEC, F.EIG_LDS_MAXN_VAL


def match(a, b):
    d = np.abs(a[:, None] - b[None, :])
    return max(d.min(axis=1).max(), d.min(axis=0).max())


def check(name, A, vectors=True):
    n = A.shape[0]
    nA = np.linalg.norm(A)
    lam_ref, V_ref = np.linalg.eig(A)
    kappa = min(float(np.linalg.cond(V_ref)), 1e8)
    wr, wi, V, iters, status = R.eig_general(A, vectors)
    assert status == R.KP_OK, name
    lam = wr + 1j * wi
    assert match(lam, lam_ref) <= 16 * kappa * n * EPS * nA, name
    s = 16 * n * EPS * nA
    assert abs(lam.sum() - np.trace(A)) <= s and abs((lam * lam).sum() - np.trace(A @ A)) <= s * nA, name
    assert math.fsum(wi) == 0.0, name
    j = 0
    while j < n:
        if wi[j] != 0.0:
            assert wi[j] > 0.0 and wi[j + 1] == -wi[j] and wr[j + 1] == wr[j], (name, j)
            j += 2
        else:
            j += 1
    if vectors:
        Vc = R.complex_vectors(wi, V)
        r, r_l = R.residual(A, lam, Vc), R.residual(A, lam_ref, V_ref)
        print(f"{name}: r {r:.3f} r_lapack {r_l:.3f}")
        assert r <= max(8 * r_l, 2.0), (name, r, r_l)
        if nA > 0:
            assert np.allclose(np.linalg.norm(Vc, axis=0), 1.0, rtol=0, atol=1e-14)
    return wr, wi, iters


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 32, 33, 64, L_VEC, L_VEC + 1, L_VAL, L_VAL + 1])
def test_random_kinds(kind, n):
    A = R.random_matrix(kind, n, 100 * n)
    a = check(f"{kind} n={n}", A, True)
    b = check(f"{kind} n={n}", A, False)
    assert np.allclose(a[0], b[0], rtol=0, atol=1e-12 * max(1.0, np.linalg.norm(A))) and a[2] == b[2]


@pytest.mark.parametrize("kind", R.KINDS)
def test_257_with_vectors(kind):
    check(f"{kind} n=257", R.random_matrix(kind, 257, 25700), True)


def test_512_values_only():
    check("gauss n=512", R.random_matrix("gauss", 512, 51200), False)


@pytest.mark.parametrize("name", sorted(R.fixed_cases()))
def test_fixed_small_cases(name):
    A = R.fixed_cases()[name]
    wr, wi, iters = check(name, A, True)
    check(name, A, False)
    if name == "complex_pair_2":
        assert wi[0] > 0 and wi[1] < 0
    if name == "cyclic_7":
        assert iters >= 10
    if name in ("zero_3", "identity_4", "triu_6"):
        assert iters == 0


def test_the_exceptional_shift_is_what_gets_the_cyclic_shift_through(monkeypatch):
    """Without iterations 10 and 20 taking another shift the double shift stagnates on a cyclic shift until the cap."""
    A = R.cyclic(4)
    assert R.eig_general(A, False)[4] == R.KP_OK
    H = A.copy()
    R.hessenberg(H, None)
    wr, wi = np.zeros(4), np.zeros(4)
    real_hqr = R.hqr

    def hqr_without(H, Z, wr, wi):
        # the same iteration with the exceptional iterations out of reach
        monkeypatch.setattr(R, "MAX_ITER", 9)
        try:
            return real_hqr(H, Z, wr, wi)
        finally:
            monkeypatch.setattr(R, "MAX_ITER", 30)
    total, ok, _ = hqr_without(H, None, wr, wi)
    assert not ok and total == 9


@pytest.mark.parametrize("n", [16, 33, 64, L_VEC + 1, L_VAL + 1])
def test_balancing(n):
    S, Cj = R.random_matrix("stable", n, 100 * n), R.random_matrix("conj", n, 100 * n)
    a, b = R.eig_general(S, False), R.eig_general(Cj, False)
    assert match(a[0] + 1j * a[1], b[0] + 1j * b[1]) <= 1e-12 * 0.8
    H = Cj.copy()
    scale = R.balance(H)
    assert np.array_equal(H * scale[None, :] ** -1 * scale[:, None], Cj)          # powers of two: exact
    assert np.all(np.log2(scale) == np.round(np.log2(scale)))


def test_non_finite_input():
    A = np.eye(3)
    A[1, 2] = np.inf
    wr, wi, V, iters, status = R.eig_general(A, True)
    assert status == R.KP_ERR_NOT_CONVERGED and np.all(np.isnan(wr)) and np.all(np.isnan(wi)) and np.all(np.isnan(V))


@pytest.mark.parametrize("vectors", [True, False])
def test_a_matrix_at_the_cap_is_nan_with_its_status(monkeypatch, vectors):
    """The cyclic shift with the cap lowered below the first exceptional shift: every output NaN, the iterations counted."""
    monkeypatch.setattr(R, "MAX_ITER", 9)
    wr, wi, V, iters, status = R.eig_general(R.cyclic(4), vectors)
    assert status == R.KP_ERR_NOT_CONVERGED and iters == 9
    assert np.all(np.isnan(wr)) and np.all(np.isnan(wi)) and (V is None if not vectors else np.all(np.isnan(V)))
