"""kp_lift_kernel (csrc/kp_context.hip) in every launch plan, descriptor path, fourier evaluation and block kind, against the
long-double lift of tests/_lift_reference.py (every column from its definition; the trigonometric argument in double, as the
reference program forms it).

Tolerance: the lift tolerance of test_gpu_fit.py, 1e-13 absolute, times max(1, max|reference column|) - Hermite columns and
their projections exceed 1.  T = 256 num_cu rows is where kp_lift_dev_ld goes from 16 to 64 points per workgroup (65 536 on an
MI355X).  Every case first asserts, through the restatement of csrc/kp_lift_plan.h in _lift_reference.py, that it lands in the
regime it is named for: points per workgroup (LT), column descriptors staged in LDS or read from global memory, and which of the
four fourier evaluations the FULL / ECON / ROW lifts take (fourier-only loop, packed table, unpacked table, generic sin / cos).
Dictionaries of more than 64 columns are compared, at the big sizes, on the first 128 rows, the last 128 and 2048 rows drawn
from a fixed seed, and checked finite everywhere; everything else on every row.

Regime per case (points per workgroup, descriptors, fourier evaluation - of the FULL / ECON / ROW lifts where they differ) and the
worst |device - reference| / max(1, max|column|) of the FULL / ECON / ROW lifts over the case's row counts, as measured on the
MI355X (the bound is 1e-13; no case needs more; the projected dictionaries are the largest, a sum of up to 364 terms):
  A-bilinear-fourier2         LT 64  staged    fourier-only / fourier-only / packed table 1.7e-16 / 1.7e-16 / 2.0e-16
  A-bilinear-poly3-pcs        LT 64  staged    -                                          1.1e-16 / 4.7e-16 / 5.2e-16
  A-linear-poly2-at           LT 64  staged    -                                          5.6e-17 / 5.6e-17 / 5.6e-17
  A-linear-poly2-below        LT 16  staged    -                                          5.6e-17 / 5.6e-17 / 5.6e-17
  A-linear-poly2-ragged       LT 64  staged    -                                          5.6e-17 / 5.6e-17 / 5.6e-17
  A-linear10-poly3-pcs        LT 64  staged    -                                          1.1e-16 / 1.1e-15 / 1.1e-15
  A-linear11-poly3-pcs        LT 16  staged    -                                          1.1e-16 / 1.3e-15 / 1.3e-15
  A-nonlinear-poly2-gaussian3 LT 64  staged    -                                          1.2e-16 / 1.2e-16 / 1.2e-16
  B-fourier1-8vars            LT 16  staged    fourier-only                               3.2e-16 / 3.2e-16 / 3.2e-16
  B-fourier1-9vars            LT 16  unstaged  unpacked table                             2.5e-16 / 2.5e-16 / 2.5e-16
  B-fourier1-fourier2         LT 16  staged    generic                                    1.4e-16 / 1.4e-16 / 1.4e-16
  B-fourier1-nonlinear        LT 16  staged    fourier-only                               1.7e-16 / 1.7e-16 / 1.7e-16
  B-fourier1-twice            LT 16  staged    fourier-only                               1.2e-16 / 1.2e-16 / 1.2e-16
  B-fourier2-2vars            LT 16  staged    fourier-only                               1.4e-16 / 1.4e-16 / 1.4e-16
  B-fourier2-pcs              LT 16  staged    fourier-only / packed table / packed table 1.4e-16 / 4.9e-16 / 4.9e-16
  B-fourier7-1var             LT 16  staged    fourier-only                               6.6e-17 / 6.6e-17 / 6.6e-17
  B-fourier8-2vars            LT 16  staged    unpacked table                             1.5e-16 / 1.5e-16 / 1.5e-16
  B-fourier9-2vars            LT 16  staged    generic                                    1.5e-16 / 1.5e-16 / 1.5e-16
  B-poly2-fourier2-bilinear   LT 16  staged    packed table                               1.4e-16 / 1.4e-16 / 1.6e-16
  B-poly2-fourier2-linear     LT 16  staged    packed table                               1.4e-16 / 1.4e-16 / 1.4e-16
  B-poly2-fourier2-nonlinear  LT 16  staged    packed table                               1.9e-16 / 1.9e-16 / 1.9e-16
  C-five-bilinear             LT 16  staged    packed table                               1.5e-16 / 1.5e-16 / 1.5e-16
  C-five-bilinear-pcs         LT 16  staged    packed table                               1.5e-16 / 5.5e-16 / 5.5e-16
  C-five-linear               LT 16  staged    packed table                               1.5e-16 / 1.5e-16 / 1.5e-16
  C-five-linear-pcs           LT 16  staged    packed table                               1.5e-16 / 5.5e-16 / 5.5e-16
  C-five-nonlinear            LT 16  staged    packed table                               1.7e-16 / 1.7e-16 / 1.7e-16
  C-five-nonlinear-pcs        LT 16  staged    packed table                               1.7e-16 / 3.7e-16 / 3.7e-16
  C-fourier_sparser3-2vars    LT 16  staged    -                                          1.4e-16 / 1.4e-16 / 1.4e-16
  C-hermite5-3vars            LT 16  staged    -                                          4.3e-16 / 4.3e-16 / 4.3e-16
  C-poly2-32vars              LT 16  staged    -                                          5.5e-17 / 5.5e-17 / 5.5e-17
  C-poly3-9vars               LT 16  staged    -                                          9.9e-17 / 9.9e-17 / 9.9e-17

Row independence: the same points in a permuted order give the same permutation of the output, bit for bit (one case each of
A, B and C).  Refusals: by return code and message, and a valid lift on the same context succeeds afterwards.  kp_fit_refine at
T + 37 pairs lifts Px and Py with 64 points per workgroup: one step from the device's own K against K + G^-1 Px'(Py - Px K)
formed in long double from the reference lift; the tolerance is the larger of the normal-equation bound of test_gpu_fit.py (1e-9
relative) and twice that reference's own distance from the QR solution (measured: that distance 1.3e-15 at max|K| = 1.02, so the
bound is 1.02e-9; the device's step is 6.1e-17 from the long-double one, its unrefined K 1.5e-15).
"""
import ctypes as C

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from koopman_realizations_amd import device as kdev
from oracle import koopman_oracle as ko
from conftest import synth_pairs
import _lift_reference as lr
from test_gpu_fit import make_basis

pytestmark = pytest.mark.gpu

TOL = 1e-13


@pytest.fixture(scope="module")
def num_cu(ctx):
    return ctx.info()["num_cu"]


def assert_regime(c, rows, num_cu):
    p = lr.plan(c.mt, c.nz, c.m, c.blocks, c.k, rows, num_cu)
    assert p["error"] is None and p["lt"] == c.lt and bool(p["stage_cols"] & 1) == c.staged, p
    assert tuple(lr.fourier_path(p, c.mt, c.blocks, c.k, w) for w in (lr.FULL, lr.ECON, lr.ROW)) == c.path, p


def device_lifts(b, c, zeta, u):
    uv = u if c.mt == "nonlinear" else None
    return {"FULL": b.lift(F.LIFT_FULL, zeta, uv), "ECON": b.lift(F.LIFT_ECON, zeta, uv), "ROW": b.lift(F.LIFT_ROW, zeta, u)}


def reference_lifts(dic, c, zeta, u):
    V = np.hstack([zeta, u]) if c.mt == "nonlinear" else zeta
    return {"FULL": lr.lift_full_ld(dic.basis, V), "ECON": lr.econ_ld(dic, V), "ROW": lr.rows_ld(dic, zeta, u)}


@pytest.mark.parametrize("name", sorted(lr.CASES))
def test_lift_against_the_long_double_reference(ctx, num_cu, name):
    c = lr.CASES[name]
    dic = lr.case_dictionary(c)
    b = make_basis(ctx, dic)
    assert (b.nvars, b.nfull, b.N, b.W) == (c.nvars, dic.basis.nfull, dic.N, dic.W)
    for spec in c.rows:
        rows = lr.row_count(spec, num_cu)
        assert_regime(c, rows, num_cu)
        zeta, u = lr.case_points(c, rows)
        got = device_lifts(b, c, zeta, u)
        if rows > 4096 and b.nfull > 64:
            idx = np.unique(np.concatenate([np.arange(128), np.arange(rows - 128, rows), np.random.default_rng(17).integers(0, rows, 2048)]))
        else:
            idx = np.arange(rows)
        ref = reference_lifts(dic, c, zeta[idx], u[idx])
        for what in ("FULL", "ECON", "ROW"):
            g, r = got[what], ref[what]
            assert g.shape == (rows, r.shape[1]) and np.isfinite(g).all()
            scale = np.maximum(1.0, np.abs(r).max(axis=0))
            worst = float((np.abs(g[idx] - r) / scale).max())
            print(f"LIFT {name} rows={rows} {what} width={g.shape[1]} max|column|={float(scale.max()):.3g} worst error / scale = {worst:.3e}")
            assert worst <= TOL, (name, rows, what, worst)


@pytest.mark.parametrize("name", ["A-bilinear-poly3-pcs", "B-poly2-fourier2-bilinear", "C-five-bilinear-pcs"])
def test_rows_do_not_depend_on_their_position_in_the_batch(ctx, num_cu, name):
    c = lr.CASES[name]
    b = make_basis(ctx, lr.case_dictionary(c))
    rows = lr.row_count(c.rows[-1], num_cu)
    assert_regime(c, rows, num_cu)
    zeta, u = lr.case_points(c, rows)
    perm = np.random.default_rng(23).permutation(rows)
    first, again = device_lifts(b, c, zeta, u), device_lifts(b, c, zeta[perm], u[perm])
    for what in first:
        assert np.array_equal(again[what], first[what][perm]), what


def small_valid_lift(ctx):
    """A lift that must still work after a refusal on the same context."""
    dic = ko.build_dictionary("linear", 2, 1, ["poly"], [2])
    z = np.random.default_rng(1).uniform(-1, 1, (5, 2))
    np.testing.assert_allclose(make_basis(ctx, dic).lift(F.LIFT_FULL, z), ko.lift_full(dic.basis, z), atol=TOL, rtol=0)


def refused(ctx, message, call):
    with pytest.raises(F.KoopmanHipError) as e:
        call()
    assert e.value.code == F.KP_ERR_ARG and message in str(e.value), str(e.value)
    small_valid_lift(ctx)


def test_lift_refuses_a_projection_too_wide_for_the_lds(ctx, num_cu):
    c = lr.CASES["B-fourier1-9vars"]
    assert lr.plan(c.mt, c.nz, c.m, c.blocks, 1, 17, num_cu)["error"] == "kp_lift: dictionary too large for the LDS staging of the pcs projection"
    dic = lr.case_dictionary(c)
    dic.pcs = np.zeros((dic.basis.nfull, 1))
    dic.pcs[0, 0] = 1.0
    b = make_basis(ctx, dic)
    zeta, u = lr.case_points(c, 17)
    for what in (F.LIFT_ECON, F.LIFT_ROW):
        refused(ctx, "kp_lift: dictionary too large for the LDS staging of the pcs projection", lambda: b.lift(what, zeta, u))


def test_basis_create_refusals(ctx):
    refused(ctx, "kp_basis_create: too many variables (max 32)", lambda: kra.Basis(ctx, "linear", 33, 1, []))
    refused(ctx, "kp_basis_create: too many variables (max 32)", lambda: kra.Basis(ctx, "nonlinear", 31, 2, []))
    refused(ctx, "kp_basis_create: fourier degree < 1", lambda: kra.Basis(ctx, "linear", 2, 1, [("fourier", 0)]))
    refused(ctx, "kp_basis_create: fourier block too large", lambda: kra.Basis(ctx, "linear", 13, 1, [("fourier", 1)]))      # 3^13 > 1e6

    def negative_count():
        d, keep = kdev.basis_desc("linear", 2, 1, [("poly", np.array([[2, 0], [1, 1], [0, 2]], dtype=np.uint8))])
        keep[1][0] = -1
        h = F.vp()
        F.check(F.lib().kp_basis_create(ctx.handle, C.byref(d), C.byref(h)), ctx.handle)
    refused(ctx, "kp_basis_create: negative block count", negative_count)


def test_lift_requires_u_where_the_layout_has_it_and_takes_no_rows(ctx):
    z = np.random.default_rng(2).uniform(-1, 1, (5, 2))
    for mt in ("linear", "bilinear", "nonlinear"):
        dic = ko.build_dictionary(mt, 2, 1, ["poly"], [2])
        b = make_basis(ctx, dic)
        refused(ctx, "kp_lift: u required", lambda: b.lift(F.LIFT_ROW, z))
        if mt == "nonlinear":
            refused(ctx, "kp_lift: u required", lambda: b.lift(F.LIFT_FULL, z))
        for what, width in ((F.LIFT_FULL, b.nfull), (F.LIFT_ECON, b.N), (F.LIFT_ROW, b.W)):
            out = b.lift(what, np.zeros((0, 2)), np.zeros((0, 1)))
            assert out.shape == (0, width)
    small_valid_lift(ctx)


def test_fit_refine_above_the_threshold_matches_one_step_in_long_double(ctx, num_cu):
    Ns = 256 * num_cu + 37
    pairs = synth_pairs(Ns, 2, 1, seed=9)
    dic = ko.build_dictionary("bilinear", 2, 1, ["poly"], [2])
    assert lr.plan("bilinear", 2, 1, lr.block_sizes(2, ["poly"], [2]), 0, Ns, num_cu)["lt"] == 64
    b = make_basis(ctx, dic)
    snaps = kra.Snapshots(ctx, pairs["alpha"], pairs["beta"], pairs["u"])
    K0 = kra.fit(ctx, b, snaps)[0]
    K1 = kra.fit_refine(ctx, b, snaps, K0, 1)
    Px, Py = lr.rows_ld(dic, pairs["alpha"], pairs["u"]), lr.rows_ld(dic, pairs["beta"], pairs["u"])
    K0l = K0.astype(lr.LD)
    Kref = K0l + lr.solve_ld(Px.T @ Px, Px.T @ (Py - Px @ K0l))
    Kq = np.linalg.lstsq(Px.astype(np.float64), Py.astype(np.float64), rcond=None)[0]
    scale = max(1.0, np.abs(Kq).max())
    measured = float(np.abs(Kref - Kq).max())
    tol = max(1e-9 * scale, 2.0 * measured)
    err = float(np.abs(K1 - Kref).max())
    print(f"REFINE Ns={Ns} W={b.W} |Kref - Kqr| = {measured:.3e} scale = {scale:.3g} tol = {tol:.3e} |K1 - Kref| = {err:.3e} |K0 - Kref| = {float(np.abs(K0l - Kref).max()):.3e}")
    assert err <= tol
