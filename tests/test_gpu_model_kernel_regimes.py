"""GPU tests of the model-extraction entry points in every dispatch regime: kp_rollout, kp_rollout_nl, kp_model_project
(csrc/kp_more.hip) and kp_sym_eig (csrc/kp_eig.hip), each against a plain reference of the same operation.

1. kp_rollout against the long-double recurrence of tests/_rollout_reference.py, whose case table walks the regimes the host
   code picks among (one wave / 256 threads, A staged or not, B staged or not, full or shortened chunks, N > 256, m = 0) with
   lengths on both sides of a chunk boundary.  1e-12 of the step's inf-norm (the float64 recurrence itself: 7e-15,
   tests/test_rollout_reference.py; the device, measured over all cases: 1.0e-14); Y[0] is z0 bit for bit; batches of five
   DISTINCT models, each equal to its single call bit for bit; a rollout between queued pipelined fits.
2. kp_rollout_nl one step ahead from the device's own trajectory against the oracle's lift (a free nonlinear rollout
   amplifies rounding differences): Z[t+1] against Kf econ_full([Z[t]; U[t]]) within 1e-12 max(1, |.|) - a product of at most
   715 terms with |psi| <= 1 rounds within 715 eps = 1.6e-13.
3. kp_model_project against the literal get_model on the DATA (M' = L \\ R by QR, not from the Grams) on both sides of every
   regime boundary of its Cholesky solve (n <= 352, <= 512, wider), with m = 0, and with a rank-deficient L.  1e-8 max(1,
   |want|), the project's bound for this routine; measured at most 4.0e-12 (M), 5.9e-15 (M A), cond(L) <= 846.
4. kp_sym_eig beyond decaying covariances: clustered, indefinite, rank-one, diagonal, zero, tiny, zero-diagonal matrices at any
   scale; n = 1023 and 1024 where the tables of the multi-workgroup kernel are exactly full; the one-workgroup form above
   n = 40 in a fresh interpreter (KP_EIG_ONE_WG is read once per process).
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from test_gpu_fit import make_basis
from conftest import synth_pairs
import _rollout_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. kp_rollout ----------------------------------------------------------------------------------------------------------
def _mt(bilinear):
    return "bilinear" if bilinear else "linear"


def _check_rollout(Y, c, label):
    Z, n_out = c["Z"], c["n_out"]
    assert Y.shape == (Z.shape[0], n_out)
    assert np.array_equal(Y[0], c["z0"][:n_out]), label                     # bit for bit
    norm = np.abs(Z).max(axis=1).astype(np.float64)
    err = np.abs(Y - Z[:, :n_out]).max(axis=1).astype(np.float64) / norm
    print("%s: worst step %d, relative error %.2e" % (label, int(err.argmax()), err.max()))
    assert err.max() <= 1e-12, (label, int(err.argmax()), err.max())


@pytest.mark.parametrize("name,T", [(n, T) for n in sorted(rr.CASES) for T in rr.CASES[n][4]])
def test_rollout_matches_the_long_double_recurrence(ctx, name, T):
    c = rr.case(name, T)
    Y = ctx.rollout(_mt(c["bilinear"]), c["A"], c["B"], c["z0"], c["U"], c["n_out"])
    _check_rollout(Y, c, "case %s T %d" % (name, T))


@pytest.mark.parametrize("name,T", [(n, T) for n in sorted(rr.CASES) if rr.CASES[n][7] for T in rr.CASES[n][4]])
def test_rollout_batch_of_distinct_models(ctx, name, T):
    """Five models that differ in A, B, z0 and U: a wrong per-model offset of any of them, or of Y, gives another model's
    trajectory.  Every member against its own reference, and bit for bit equal to the single call of that model."""
    cs = [rr.case(name, T, i) for i in range(rr.BATCH)]
    mt, n_out = _mt(cs[0]["bilinear"]), cs[0]["n_out"]
    Yb = ctx.rollout(mt, np.stack([c["A"] for c in cs]), np.stack([c["B"] for c in cs]), np.stack([c["z0"] for c in cs]),
                     np.stack([c["U"] for c in cs]), n_out)
    assert Yb.shape == (rr.BATCH, T, n_out)
    for i, c in enumerate(cs):
        _check_rollout(Yb[i], c, "case %s T %d member %d" % (name, T, i))
        Y1 = ctx.rollout(mt, c["A"], c["B"], c["z0"], c["U"], n_out)
        assert np.array_equal(Yb[i], Y1), (name, T, i)


def test_rollout_between_queued_pipelined_fits(ctx):
    """kp_rollout shares workspace slot 6 and the event pair with the fits: it completes the queue first.  Five pipelined fits
    on a small bilinear dictionary, a rollout (case a), then the results: the rollout against its reference, every K against
    the synchronous fit of the same snapshots within the 1e-11 max|K| pipelined fits are held to elsewhere."""
    b = kra.Basis(ctx, "bilinear", 3, 1, [("poly", kra.poly_exponent_table(3, 2)[3:])])
    pairs = [synth_pairs(600, 3, 1, seed=900 + i) for i in range(5)]
    snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in pairs]
    Kref = [kra.fit(ctx, b, s)[0] for s in snaps]
    c = rr.case("a", 257)
    for s in snaps:
        kra.fit(ctx, b, s, fetch=False)
    Y = ctx.rollout("linear", c["A"], c["B"], c["z0"], c["U"], c["n_out"])
    ctx.synchronize()
    _check_rollout(Y, c, "case a T 257 between queued fits")
    for q in range(5):
        K = ctx.fit_result(q, b.W)
        err = np.abs(K - Kref[q]).max()
        print("queued fit %d: |K - K_sync| %.2e (bound %.2e)" % (q, err, 1e-11 * np.abs(Kref[q]).max()))
        assert err <= 1e-11 * np.abs(Kref[q]).max(), q


# ---- 2. kp_rollout_nl -------------------------------------------------------------------------------------------------------
NL_T = (1, 2, 25)
NL_CASES = ("poly2", "poly4", "pcs", "fourier", "gaussian")


@functools.lru_cache(maxsize=None)
def _nl_dictionary(name):
    rng = np.random.default_rng(50)
    if name == "poly2":              # the smallest case, k_pcs == 0
        nz, m, basis, pcs = 2, 1, ko.make_basis(3, ["poly"], [2]), None
    elif name == "poly4":            # nfull = N = 715: both thread-stride loops of the kernel wrap (256 threads)
        nz, m, basis, pcs = 6, 3, ko.make_basis(9, ["poly"], [4]), None
    elif name == "pcs":              # the three branches of the econ layout: variables, projections, trailing 1
        nz, m, basis = 6, 3, ko.make_basis(9, ["poly"], [3])
        pcs = np.linalg.qr(rng.standard_normal((basis.nfull, 20)))[0]
    elif name == "fourier":
        nz, m, basis, pcs = 2, 1, ko.make_basis(3, ["fourier"], [1]), None
    else:
        nz, m, basis, pcs = 2, 1, ko.make_basis(3, ["gaussian"], [5], [rng.uniform(-1, 1, (3, 5))]), None
    return ko.Dictionary("nonlinear", nz, m, basis, pcs)


def _nl_model(dic, T, seed):
    """Kf, zeta0, U with every row of Kf scaled so that |Kf econ_full(v)|_inf <= 0.9 for EVERY v in the box [-1, 1]^(nzeta+m):
    there each dictionary function is at most 1 in size, a projection pcs_j' psi at most |pcs_j|_1."""
    rng = np.random.default_rng(seed)
    nz, m, N = dic.nzeta, dic.m, dic.N
    bound = np.ones(N)
    if dic.pcs is not None:
        bound[nz + m:nz + m + dic.pcs.shape[1]] = np.abs(dic.pcs).sum(axis=0)
    Kf = rng.standard_normal((nz, N))
    Kf[:, :nz + m] *= 5.0                                  # the next point depends visibly on the current one
    Kf *= 0.9 / (np.abs(Kf) @ bound)[:, None]
    return Kf, rng.uniform(-0.9, 0.9, nz), rng.uniform(-1, 1, (T, m))


def _check_nl(dic, Kf, zeta0, U, Z, label):
    """One step ahead from the device's own trajectory (measured figures: test_rollout_nl_one_step_ahead)."""
    T = U.shape[0]
    assert Z.shape == (T, dic.nzeta) and np.array_equal(Z[0], zeta0), label
    assert np.isfinite(Z).all() and np.abs(Z).max() <= 0.9, label
    if T == 1:
        return 0.0
    want = ko.econ_full(dic, np.hstack([Z[:-1], U[:-1]])) @ Kf.T
    assert np.abs(want).max() <= 0.9, label
    err = np.abs(Z[1:] - want).max()
    print("%s: one-step error %.2e, |zeta| %.3g ... %.3g" % (label, err, np.abs(Z).max(axis=1).min(), np.abs(Z).max()))
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (label, err)
    return err


@pytest.mark.parametrize("T", NL_T)
@pytest.mark.parametrize("name", NL_CASES)
def test_rollout_nl_one_step_ahead(ctx, name, T):
    """Bound 1e-12 max(1, |want|), from the rounding analysis in the module docstring; measured on the MI355X at most 5.6e-17
    (poly2, fourier, gaussian), 3.1e-17 (poly4), 1.4e-17 (pcs) - the rows of Kf are scaled to an l1 weight of 0.9, so the
    sums are far smaller than their worst case.  No case needed a measured bound."""
    dic = _nl_dictionary(name)
    b = make_basis(ctx, dic)
    assert (b.nfull, b.N) == (dic.basis.nfull, dic.N)
    Kf, zeta0, U = _nl_model(dic, T, 60 + T)
    Z = ctx.rollout_nl(b, Kf, zeta0, U)
    _check_nl(dic, Kf, zeta0, U, Z, "%s T %d" % (name, T))


@pytest.mark.parametrize("name", ["poly2", "pcs"])
def test_rollout_nl_batch_of_distinct_models(ctx, name):
    dic = _nl_dictionary(name)
    b = make_basis(ctx, dic)
    T = 25
    mdl = [_nl_model(dic, T, 70 + i) for i in range(4)]
    Zb = ctx.rollout_nl_batch(b, np.stack([k for k, _, _ in mdl]), np.stack([z for _, z, _ in mdl]), np.stack([u for _, _, u in mdl]))
    assert Zb.shape == (4, T, dic.nzeta)
    for i, (Kf, zeta0, U) in enumerate(mdl):
        _check_nl(dic, Kf, zeta0, U, Zb[i], "%s batch member %d" % (name, i))
        assert np.array_equal(Zb[i], ctx.rollout_nl(b, Kf, zeta0, U)), (name, i)


# ---- 3. kp_model_project ----------------------------------------------------------------------------------------------------
MP_SHAPES = [(1, 0), (1, 1), (2, 1), (17, 3), (40, 0), (130, 3), (352, 2), (353, 2), (520, 2)]


@functools.lru_cache(maxsize=None)
def _mp_data(N, m, seed):
    rng = np.random.default_rng(seed)
    W = N + m
    P = rng.standard_normal((3 * W + 10, W))
    Y = P @ (0.3 * rng.standard_normal((W, W)) / np.sqrt(W)) + 0.01 * rng.standard_normal((3 * W + 10, W))
    return P, Y, _lstsq(P, Y)


def _lstsq(X, Y):
    """X \\ Y on the data: Householder QR where X has full column rank (cond <= 1e3 here: what MATLAB's `\\` does, and a
    fraction of the time of the SVD driver at 1576 x 522), numpy's minimum-norm lstsq where it has not."""
    Q, R = np.linalg.qr(X)
    d = np.abs(np.diag(R))
    if d.min() <= 1e-10 * d.max():
        return np.linalg.lstsq(X, Y, rcond=None)[0]
    return np.linalg.solve(R, Q.T @ Y)


def _mp_reference(P, Y, K, N):
    """The literal get_model (Ksysid.m:1206-1225) on the data, not on the Grams: L = [Px U] K(:, 1:N), M' = L \\ R."""
    L = P @ K[:, :N]
    M = _lstsq(L, Y[:, :N]).T
    A, B = K[:N, :N].T, K[N:, :N].T
    return L, M, A, B


def _project(ctx, K, G, Cm, N, m):
    """kp_model_project through the C ABI with a B buffer that is never empty: with m = 0 it must come back untouched."""
    K = F.fcol(K); G = F.fcol(G); Cm = F.fcol(Cm)
    A = np.zeros((N, N), order="F"); M = np.zeros((N, N), order="F")
    B = np.full((N, max(m, 1)), 7.25, order="F")
    F.check(F.lib().kp_model_project(ctx.handle, F.dptr(K), F.dptr(G), F.dptr(Cm), N, m, F.dptr(A), F.dptr(B), F.dptr(M)), ctx.handle)
    if m == 0:
        assert (B == 7.25).all()
        return A, np.zeros((N, 0)), M
    return A, B, M


@pytest.mark.parametrize("N,m", MP_SHAPES)
def test_model_project_matches_the_literal_get_model(ctx, N, m):
    P, Y, K = _mp_data(N, m, 1000 + N)
    L, M, A, B = _mp_reference(P, Y, K, N)
    A_out, B_out, M_out = _project(ctx, K, P.T @ P, P.T @ Y, N, m)
    print("N %d m %d: cond(L) %.3g" % (N, m, np.linalg.cond(L)))
    for what, got, want in (("M A", A_out, M @ A), ("M B", B_out, M @ B), ("M", M_out, M)):
        if want.size == 0:
            assert got.shape == want.shape
            continue
        err = np.abs(got - want).max()
        print("N %d m %d %s: error %.2e (bound %.2e)" % (N, m, what, err, 1e-8 * max(1.0, np.abs(want).max())))
        assert err <= 1e-8 * max(1.0, np.abs(want).max()), (what, err)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("N,m", [(8, 1), (40, 2), (130, 3)])
def test_model_project_with_a_rank_deficient_L(ctx, N, m, seed):
    """K(:, N) = K(:, 1): two equal columns of L, M is not unique.  What is: the residual of the least-squares problem (the
    (1 + 1e-5) of tests/test_gpu_continuous.py for this routine), and A_out = M_out A, B_out = M_out B."""
    P, Y, K = _mp_data(N, m, 2000 + 10 * N + seed)
    K = K.copy()
    K[:, N - 1] = K[:, 0]
    L, M, A, B = _mp_reference(P, Y, K, N)
    assert np.linalg.matrix_rank(L) == N - 1
    A_out, B_out, M_out = _project(ctx, K, P.T @ P, P.T @ Y, N, m)
    assert np.isfinite(M_out).all() and np.isfinite(A_out).all() and np.isfinite(B_out).all()
    R = Y[:, :N]
    r_dev, r_ref = np.linalg.norm(L @ M_out.T - R), np.linalg.norm(L @ M.T - R)
    print("N %d m %d seed %d: residual %.6g against lstsq's %.6g (ratio - 1 = %.2e), max|M| %.3g" % (N, m, seed, r_dev, r_ref, r_dev / r_ref - 1, np.abs(M_out).max()))
    assert r_dev <= (1 + 1e-5) * r_ref
    for got, want in ((A_out, M_out @ A), (B_out, M_out @ B)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- 4. kp_sym_eig ----------------------------------------------------------------------------------------------------------
EIG_N = (3, 7, 40, 41, 128, 257)
EIG_CLASSES = ("clusters", "wishart", "identity_noise", "rank_one", "diagonal", "zero", "tiny", "zero_diag_1", "zero_diag_1e20",
               "zero_diag_1e-20")


def eig_matrix(kind, n):
    rng = np.random.default_rng(1000 * EIG_CLASSES.index(kind) + n if kind in EIG_CLASSES else n)
    if kind == "decaying":           # the covariance of test_gpu_models.test_sym_eig_matches_lapack
        X = rng.standard_normal((max(4 * n, 50), n)) * np.logspace(0, -6, n)
        return np.atleast_2d(np.cov(X, rowvar=False))
    if kind == "clusters":           # three clusters of equal eigenvalues, indefinite
        Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        lam = np.repeat([3.0, 1.0, -2.0], (n + 2) // 3)[:n]
        S = (Q * lam) @ Q.T
        return (S + S.T) / 2
    if kind == "wishart":
        X = rng.standard_normal((4 * n, n))
        return X.T @ X / (4 * n)
    if kind == "identity_noise":
        E = rng.standard_normal((n, n))
        return np.eye(n) + 1e-14 * (E + E.T)
    if kind == "rank_one":
        v = rng.standard_normal(n)
        return np.outer(v, v)
    if kind == "diagonal":
        return np.diag(rng.standard_normal(n))
    if kind == "zero":
        return np.zeros((n, n))
    if kind == "tiny":
        X = rng.standard_normal((n, n))
        return 1e-200 * (X @ X.T)
    H = rng.standard_normal((n, n))
    H = H + H.T
    np.fill_diagonal(H, 0.0)
    return float(kind.split("_")[-1]) * H


def _check_eig(S, w, V, sweeps, label):
    """The bounds of test_gpu_models.test_sym_eig_matches_lapack: eigenvalues 1e-13 scale max(1, n / 50), residual 1e-12 scale,
    orthogonality 1e-12 - with scale the spectral radius (0 for the zero matrix: everything exact)."""
    n = S.shape[0]
    wl = np.linalg.eigvalsh(S)[::-1]
    scale = np.abs(wl).max()
    e_w, e_r, e_o = np.abs(w - wl).max(), np.abs(S @ V - V * w).max(), np.abs(V.T @ V - np.eye(n)).max()
    unit = scale if scale > 0 else 1.0
    print("%s: sweeps %d, eigenvalues %.2e, residual %.2e (both / scale), orthogonality %.2e" % (label, sweeps, e_w / unit, e_r / unit, e_o))
    assert 1 <= sweeps <= 30, label
    assert np.isfinite(w).all() and np.isfinite(V).all(), label
    assert e_w <= 1e-13 * scale * max(1, n / 50), (label, e_w / unit, sweeps)
    assert e_r <= 1e-12 * scale, (label, e_r / unit, sweeps)
    assert e_o <= 1e-12, (label, e_o, sweeps)
    return wl, scale


@pytest.mark.parametrize("n", EIG_N)
@pytest.mark.parametrize("kind", EIG_CLASSES)
def test_sym_eig_input_classes(ctx, kind, n):
    """One-workgroup form for n <= 40, multi-workgroup form above (n = 41, 257: odd, one index idle every round).
    zero_diag_1e-20 failed while the convergence scale came from the diagonal alone: the scale fell back to 1.0, every entry
    was below 1e-15 of it and the solver returned after ONE sweep with eigenvalue errors of 2.9e-4 (n = 3), 0.37 (7), 0.21
    (40), 0.20 (41), 0.21 (128), 0.23 (257) of the spectral radius; with the scale from the whole matrix: at most 6.0e-14.
    All bounds are the ones of _check_eig, none was widened.  Sweeps measured on the MI355X at n = 3, 7, 40, 41, 128, 257
    (never asserted below the cap: the threshold 1e-15 scale lies below the n eps rounding floor of a flat spectrum):
      clusters          4  7 19 21 29 30    worst / bound at n = 257: eigenvalues 2.6e-13 / 5.1e-13, orthogonality 2.6e-13 / 1e-12
      wishart           4  6  9  8 10 11
      identity_noise    3  4  6  6  7  8
      rank_one          2  2  2  2  2  3
      diagonal, zero    1  1  1  1  1  1
      tiny              4  6  9  9 11 13
      zero_diag (1, 1e20, 1e-20)   4  6-7  8-9  8-9  10-11  11
    The cluster matrix reaches the cap of 30 at n = 255 ... 257 and is as accurate there as the bounds ask: kp_sym_eig
    returns KP_OK and reports the cap through `sweeps` (include/koopman_hip.h)."""
    S = eig_matrix(kind, n)
    w, V, sweeps = ctx.sym_eig(S)
    _check_eig(S, w, V, sweeps, "%s n %d" % (kind, n))
    if kind == "diagonal":           # no rotation at all: one sweep, V a permutation of the identity, the eigenvalues the entries
        assert sweeps == 1
        assert ((V == 0) | (V == 1)).all() and (V.sum(axis=0) == 1).all() and (V.sum(axis=1) == 1).all()
        assert np.array_equal(w, np.sort(np.diag(S))[::-1])
    if kind == "zero":
        assert sweeps == 1 and not w.any()


@pytest.mark.parametrize("n", [1023, 1024])
def test_sym_eig_at_the_limit_of_the_multi_workgroup_tables(ctx, n):
    """cs[] and pq[] of kp_jacobi_eig_mw_kernel hold 1024 entries: n = 1024 fills them, n = 1023 (odd) as well, with the dummy
    player."""
    S = eig_matrix("decaying", n)
    w, V, sweeps = ctx.sym_eig(S)
    _check_eig(S, w, V, sweeps, "decaying n %d" % n)


def test_sym_eig_rejects_n_above_1024(ctx):
    with pytest.raises(kra.KoopmanHipError) as e:
        ctx.sym_eig(np.eye(1025))
    assert e.value.code == F.KP_ERR_ARG


ONE_WG_N = (41, 85, 255, 256)
ONE_WG_KINDS = ("decaying", "clusters")

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from test_gpu_model_kernel_regimes import eig_matrix, ONE_WG_N, ONE_WG_KINDS
ctx = kra.Context(0)
res = {}
for kind in ONE_WG_KINDS:
    for n in ONE_WG_N:
        w, V, sweeps = ctx.sym_eig(eig_matrix(kind, n))
        res["w_%s_%d" % (kind, n)] = w; res["V_%s_%d" % (kind, n)] = V; res["s_%s_%d" % (kind, n)] = np.int64(sweeps)
err, code = "", 0
try:
    ctx.sym_eig(eig_matrix("decaying", 257))
except kra.KoopmanHipError as e:
    err, code = str(e), e.code
res["err_257"] = np.array(err); res["code_257"] = np.int64(code)
np.savez(sys.argv[2], **res)
print("EIG_ONE_WG_CHILD_OK")
"""


@pytest.fixture(scope="module")
def one_wg(tmp_path_factory):
    """Eight decompositions in the one-workgroup form.  It takes 88 ms at n = 220 and ten sweeps; n = 256 at the cap of 30 sweeps
    is 88 ms (256 / 220)^3 * 3 = 0.42 s, so the eight stay below 4 s beside the start of an interpreter and a context: 120 s is
    a limit for a child that hangs, not a time the test waits for."""
    out = str(tmp_path_factory.mktemp("eig_one_wg") / "one_wg.npz")
    env = dict(os.environ)
    env["KP_EIG_ONE_WG"] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "EIG_ONE_WG_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.mark.parametrize("n", ONE_WG_N)
@pytest.mark.parametrize("kind", ONE_WG_KINDS)
def test_sym_eig_one_workgroup_form_above_n_40(ctx, one_wg, kind, n):
    """The fallback of kp_sym_eig when the grid barrier gives up, forced by KP_EIG_ONE_WG: the same assertions, and the same
    eigenvalues as the multi-workgroup form of this process within the eigenvalue bound."""
    S = eig_matrix(kind, n)
    key = "%s_%d" % (kind, n)
    w, V, sweeps = one_wg["w_" + key], one_wg["V_" + key], int(one_wg["s_" + key])
    _, scale = _check_eig(S, w, V, sweeps, "one workgroup: %s n %d" % (kind, n))
    wm, Vm, sm = ctx.sym_eig(S)
    _check_eig(S, wm, Vm, sm, "multi workgroup: %s n %d" % (kind, n))
    assert np.abs(w - wm).max() <= 1e-13 * scale * max(1, n / 50)


def test_sym_eig_one_workgroup_form_rejects_n_above_256(one_wg):
    assert int(one_wg["code_257"]) == F.KP_ERR_ARG and "multi-workgroup" in str(one_wg["err_257"])
