"""kp_eig on the device against numpy.linalg.eig (LAPACK) of the same matrix - never against the code under test.

Cases (tests/_eig_reference.py): Gaussian, "stable" (Gaussian scaled to radius 0.8), random orthogonal (normal: kappa(V) = 1)
and the stable matrix conjugated by diag(2**k), k in [-20, 20], at n = 1, 2, 3, 5, 16, 32, 33 (both sides of the wave limit),
L, L + 1, L', L' + 1 (the header's two LDS limits: 99 with vectors, 140 values only), 257 with vectors and 512 values only,
once; and the fixed small cases.

Residual r = ||A V - V diag(lam)||_F / (n eps ||A||_F): LAPACK's own r over this list is at most 1.4, and the device must keep
r_dev <= max(8 r_lapack, 2) - room for another, equally backward-stable reflector and shift convention, not for an error that
grows with n.  Eigenvalues: in both directions within 16 kappa_2(V_lapack) n eps ||A||_F of a LAPACK eigenvalue (Bauer-Fike on
two backward-stable results); the first two power sums against tr A and tr A^2; wi sums to exactly 0; pairs adjacent, the
positive imaginary part first.

Measured on an MI355X over the whole list: the worst r_dev / max(r_lapack, 0.25) is 1.59 (Gaussian, n = 3; r_dev 1.17
against r_lapack 0.74), and the ratio does not grow with n (at most 1.06 from n = 16 to n = 257)."""
import functools
import math

import numpy as np
import pytest

import _eig_reference as R
from koopman_realizations_amd import _ffi as F

pytestmark = pytest.mark.gpu

EPS = R.EPS
L_VEC, L_VAL = F.EIG_LDS_MAXN_VEC, F.EIG_LDS_MAXN_VAL
SIZES = (1, 2, 3, 5, 16, 32, 33, L_VEC, L_VEC + 1, L_VAL, L_VAL + 1)


def raw_eig(ctx, A, vectors=True, null_v=False, nb=None, n=None):
    """kp_eig itself: (rc, wr, wi, V, iters, status) with V[b][:, j] column j of the packed real form."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim == 2:
        A = A[None]
    nb = A.shape[0] if nb is None else nb
    n = A.shape[1] if n is None else n
    Ac = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
    wr, wi = np.zeros((A.shape[0], A.shape[1])), np.zeros((A.shape[0], A.shape[1]))
    Vp = np.zeros_like(Ac)
    it, st = np.zeros(A.shape[0], dtype=np.int32), np.zeros(A.shape[0], dtype=np.int32)
    rc = F.lib().kp_eig(ctx.handle, nb, n, F.dptr(Ac), int(vectors), F.dptr(wr), F.dptr(wi),
                        None if (null_v or not vectors) else F.dptr(Vp), it.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip))
    return rc, wr, wi, (np.transpose(Vp, (0, 2, 1)) if vectors else None), it, st


def expected_regime(n, vectors):
    return 1 if n <= F.EIG_WAVE_MAX else 2 if n <= (L_VEC if vectors else L_VAL) else 3


@functools.lru_cache(maxsize=None)
def lapack(kind, n):
    """(A, lam, V, r_lapack, kappa_2(V)) - computed once per case and shared."""
    A = R.fixed_cases()[kind] if n == 0 else R.random_matrix(kind, n, 100 * n + (0 if kind in ("stable", "conj") else 1 + R.KINDS.index(kind)))
    lam, V = np.linalg.eig(A)
    A.setflags(write=False)
    return A, lam, V, R.residual(A, lam, V), float(np.linalg.cond(V))


def match(a, b):
    """The larger of the two one-sided distances between the eigenvalue sets a and b."""
    d = np.abs(a[:, None] - b[None, :])
    return max(d.min(axis=1).max(), d.min(axis=0).max())


def check_values(name, A, wr, wi, lam_ref, kappa):
    n = A.shape[0]
    nA = np.linalg.norm(A)
    lam = wr + 1j * wi
    assert np.all(np.isfinite(wr)) and np.all(np.isfinite(wi)), name
    tol = 16 * kappa * n * EPS * nA
    d = match(lam, lam_ref)
    print(f"{name}: eigenvalue distance {d:.3e} (bound {tol:.3e})")
    assert d <= tol, (name, d, tol)
    s = 16 * n * EPS * nA
    assert abs(lam.sum() - np.trace(A)) <= s, (name, "trace")
    assert abs((lam * lam).sum() - np.trace(A @ A)) <= s * nA, (name, "trace of the square")
    assert math.fsum(wi) == 0.0, name          # the exact sum: every pair cancels
    j = 0
    while j < n:
        if wi[j] != 0.0:
            assert wi[j] > 0.0 and j + 1 < n and wi[j + 1] == -wi[j] and wr[j + 1] == wr[j], (name, j)
            j += 2
        else:
            j += 1


def check_vectors(name, A, wr, wi, V, r_lapack):
    Vc = R.complex_vectors(wi, V)
    if np.linalg.norm(A) > 0:
        assert np.allclose(np.linalg.norm(Vc, axis=0), 1.0, rtol=0, atol=1e-14), name
    r = R.residual(A, wr + 1j * wi, Vc)
    print(f"{name}: r_dev {r:.3f} r_lapack {r_lapack:.3f} ratio {r / max(r_lapack, 0.25):.2f}")
    assert r <= max(8 * r_lapack, 2.0), (name, r, r_lapack)
    return r


@pytest.mark.parametrize("vectors", [True, False], ids=["vectors", "values"])
@pytest.mark.parametrize("n", SIZES)
def test_random_kinds_against_lapack(ctx, n, vectors):
    """The four kinds of one size in one call; the regime is the one that the header's limits give."""
    cases = [lapack(k, n) for k in R.KINDS]
    rc, wr, wi, V, it, st = raw_eig(ctx, np.stack([c[0] for c in cases]), vectors)
    assert rc == F.KP_OK and np.all(st == F.KP_OK)
    assert ctx.timer(F.TIMER_EIG_REGIME) == expected_regime(n, vectors)
    assert ctx.timer(F.TIMER_EIG) > 0
    for b, (kind, (A, lam, _, r_l, kappa)) in enumerate(zip(R.KINDS, cases)):
        check_values(f"{kind} n={n}", A, wr[b], wi[b], lam, kappa)
        if vectors:
            check_vectors(f"{kind} n={n}", A, wr[b], wi[b], V[b], r_l)


def test_257_with_vectors_runs_from_the_workspace(ctx):
    cases = [lapack(k, 257) for k in R.KINDS]
    rc, wr, wi, V, it, st = raw_eig(ctx, np.stack([c[0] for c in cases]), True)
    assert rc == F.KP_OK and np.all(st == F.KP_OK) and ctx.timer(F.TIMER_EIG_REGIME) == 3
    for b, (kind, (A, lam, _, r_l, kappa)) in enumerate(zip(R.KINDS, cases)):
        check_values(f"{kind} n=257", A, wr[b], wi[b], lam, kappa)
        check_vectors(f"{kind} n=257", A, wr[b], wi[b], V[b], r_l)


def test_512_values_only(ctx):
    A, lam, _, _, kappa = lapack("gauss", 512)
    rc, wr, wi, _, it, st = raw_eig(ctx, A, False)
    assert rc == F.KP_OK and st[0] == F.KP_OK and ctx.timer(F.TIMER_EIG_REGIME) == 3
    check_values("gauss n=512", A, wr[0], wi[0], lam, kappa)


@pytest.mark.parametrize("name", sorted(R.fixed_cases()))
def test_fixed_small_cases(ctx, name):
    A, lam, _, r_l, kappa = lapack(name, 0)
    for vectors in (True, False):
        rc, wr, wi, V, it, st = raw_eig(ctx, A, vectors)
        assert rc == F.KP_OK and st[0] == F.KP_OK
        if not np.all(np.isfinite(lam)) or not np.isfinite(kappa):
            kappa = 1.0
        check_values(name, A, wr[0], wi[0], lam, min(kappa, 1e8))
        if vectors:
            check_vectors(name, A, wr[0], wi[0], V[0], r_l)
    if name == "complex_pair_2":
        assert wi[0][0] > 0 and wi[0][1] < 0
    if name == "real_pair_2":
        assert np.all(wi[0] == 0)
    if name == "cyclic_7":
        assert it[0] >= 10          # the double shift stagnates on a cyclic shift: the exceptional shift has run
    if name in ("zero_3", "identity_4", "triu_6"):
        assert it[0] == 0


@pytest.mark.parametrize("n", [16, 33, 100])
def test_balancing_recovers_the_spectrum_of_a_badly_scaled_matrix(ctx, n):
    """inv(D) S D with D = diag(2**k), k in [-20, 20] has the eigenvalues of S: to 1e-12 radius on the device (LAPACK: 3e-15);
    an unbalanced solver misses by orders of magnitude."""
    S, C_ = lapack("stable", n)[0], lapack("conj", n)[0]
    rc, wr, wi, _, it, st = raw_eig(ctx, np.stack([S, C_]), False)
    assert rc == F.KP_OK and np.all(st == F.KP_OK)
    d = match(wr[0] + 1j * wi[0], wr[1] + 1j * wi[1])
    print(f"n={n}: conjugated against plain {d:.3e}")
    assert d <= 1e-12 * 0.8


@pytest.mark.parametrize("n", [5, 32])
def test_forced_regimes_agree_bit_for_bit(ctx, n, monkeypatch):
    A, lam, _, r_l, kappa = lapack("gauss", n)
    out = {}
    for regime in (2, 3):
        monkeypatch.setenv("KP_EIG_REGIME", str(regime))
        for vectors in (True, False):
            rc, wr, wi, V, it, st = raw_eig(ctx, A, vectors)
            assert rc == F.KP_OK and st[0] == F.KP_OK and ctx.timer(F.TIMER_EIG_REGIME) == regime
            out[regime, vectors] = (wr, wi, V, it)
            check_values(f"regime {regime} n={n}", A, wr[0], wi[0], lam, kappa)
            if vectors:
                check_vectors(f"regime {regime} n={n}", A, wr[0], wi[0], V[0], r_l)
    monkeypatch.delenv("KP_EIG_REGIME")
    for vectors in (True, False):
        a, b = out[2, vectors], out[3, vectors]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        if vectors:
            assert np.array_equal(a[2], b[2])
    rc, wr, wi, V, it, st = raw_eig(ctx, A, True)
    assert ctx.timer(F.TIMER_EIG_REGIME) == 1
    check_vectors(f"regime 1 n={n}", A, wr[0], wi[0], V[0], r_l)


def test_forcing_regime_2_beyond_the_lds_limit_is_ignored(ctx, monkeypatch):
    monkeypatch.setenv("KP_EIG_REGIME", "2")
    raw_eig(ctx, lapack("gauss", L_VEC + 1)[0], True)
    assert ctx.timer(F.TIMER_EIG_REGIME) == 3          # the shape does not admit 2
    raw_eig(ctx, lapack("gauss", L_VEC + 1)[0], False)
    assert ctx.timer(F.TIMER_EIG_REGIME) == 2


@pytest.mark.parametrize("n", [10, 33])
def test_a_matrix_gives_the_same_bits_alone_first_and_last_of_64(ctx, n):
    rng = np.random.default_rng(n)
    stack = rng.standard_normal((64, n, n))
    A = rng.standard_normal((n, n))
    alone = raw_eig(ctx, A, True)
    stack[0] = A
    first = raw_eig(ctx, stack, True)
    stack[0] = stack[1]
    stack[63] = A
    last = raw_eig(ctx, stack, True)
    for res, b in ((first, 0), (last, 63)):
        assert np.all(res[5] == F.KP_OK)
        for k in (1, 2, 3, 4):
            assert np.array_equal(alone[k][0], res[k][b]), (b, k)


def test_a_nan_matrix_fails_alone(ctx):
    rng = np.random.default_rng(3)
    stack = rng.standard_normal((3, 12, 12))
    good = raw_eig(ctx, stack, True)
    stack[1, 4, 7] = np.nan
    rc, wr, wi, V, it, st = raw_eig(ctx, stack, True)
    assert rc == F.KP_OK
    assert list(st) == [F.KP_OK, F.KP_ERR_NOT_CONVERGED, F.KP_OK]
    assert np.all(np.isnan(wr[1])) and np.all(np.isnan(wi[1])) and np.all(np.isnan(V[1]))
    for b in (0, 2):
        for k, x in ((1, wr), (2, wi), (3, V)):
            assert np.array_equal(good[k][b], x[b])
    stack[1, 4, 7] = np.inf
    assert list(raw_eig(ctx, stack, False)[5]) == [F.KP_OK, F.KP_ERR_NOT_CONVERGED, F.KP_OK]


def test_argument_errors_leave_the_context_usable(ctx):
    A = np.eye(4)
    big = np.zeros((1, 513, 513))
    for kwargs, M in (({"n": 0}, A), ({}, big), ({"nb": 0}, A), ({"null_v": True}, A)):
        rc = raw_eig(ctx, M, True, **kwargs)[0]
        assert rc == F.KP_ERR_ARG, kwargs
        msg = F.lib().kp_last_error(ctx.handle)
        assert msg and b"kp_eig" in msg, kwargs
    lam, V, it, st = ctx.eig(np.diag([3.0, -2.0, 1.0, 0.5]))
    assert st == F.KP_OK and np.array_equal(lam, [3.0, -2.0, 1.0, 0.5])


def test_context_eig_sorts_and_unpacks(ctx):
    A = lapack("gauss", 16)[0]
    lam, V, it, st = ctx.eig(A)
    assert st == F.KP_OK and lam.dtype == complex and V.dtype == complex
    assert np.all(np.diff(np.abs(lam)) <= 1e-15)
    assert R.residual(A, lam, V) <= 2.0
    lam2, V2, it2, st2 = ctx.eig(np.stack([A, A.T]), vectors=False)
    assert V2 is None and np.allclose(lam2[0], lam, rtol=0, atol=1e-12) and lam2.shape == (2, 16)
