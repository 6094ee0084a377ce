"""kp_qp_solve (the one-wave Goldfarb-Idnani solver of csrc/kp_qp.h, one workgroup of 64 lanes) across the whole range
its entry point admits, against the independent high-precision optimum of tests/_qp_reference.py:

- sizes n in {1, 31, 32, 33, 63, 64}, up to the largest row count the 160 KB LDS budget of qp_lds_doubles admits at
  n = 64 (920 rows; one more is refused with "too large");
- rows with 1-4 non-zeros (ELL K <= QP_KLDS: rows, norms and b copied into LDS), dense rows (K > 4: read from global
  memory), and a mix (K > 4 as well: every row from global memory);
- cond(H) from 1 to 1e8;
- degenerate vertices: more than n rows tight at the optimum, duplicated rows, anti-parallel pairs pinning a variable (the
  form of Kmpc.m:865-870), zero rows;
- infeasible problems: NaN and KP_ERR_QP_FAIL, among them 900-row problems at n = 64 whose infeasibility needs all 65
  rows of a simplex (a full active set of 64 rows and one more).

Tolerance: |x - x*|_inf <= C(kappa) eps kappa max(1, |x*|_inf), kappa = max(cond(H), cond of the optimum's KKT matrix).
C(kappa) is continuous: log-linear in log kappa through (1, 2e3), (1e4, 4.5e4), (1e6, 1.5e6), constant 1.5e6 beyond.
Worst C_meas = error / (eps kappa max(1, |x*|)) measured on the MI355X, per range of kappa, and the margin of C there:
    kappa < 2e3:  209 (920 dense rows, kappa 555)   margin 81x
    kappa ~ 1e4:  5.7e3 (n = 32, dense)            margin 7.9x (C(1e4) = 4.5e4 puts the bound at 9.99e-8 max(1, |x*|),
                                                    just under the 1e-7 of test_generic_qp_shim_on_random_problems)
    kappa = 1e6:  1.5e5 (n = 64, dense)            margin 10x
    kappa = 1e8:  1.2e5 (n = 32, dense)            margin 12x
The device loses up to ~30x more than the float64 oracle on the same problems (oracle C_meas <= 1.9e4 at kappa 1e6 - 1e8,
<= 224 at 1e4): both run Goldfarb-Idnani, but the oracle re-solves N'H^-1 N for every step, while the device keeps its
inverse Sinv by rank-1 updates and downdates and moves x incrementally, and its error accumulates over the ~n steps."""
import numpy as np
import pytest

import _qp_reference as qr
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def c_tol(kappa):
    """C(kappa) of the module docstring: continuous, so rounding of kappa near a decade cannot switch the bound."""
    return float(np.exp(np.interp(np.log(kappa), np.log([1.0, 1e4, 1e6, 1e8]), np.log([2e3, 4.5e4, 1.5e6, 1.5e6]))))


def qp_lds_doubles(n, mr):
    """csrc/kp_qp.h:qp_lds_doubles, mirrored (QP_KLDS = 4)."""
    return 3 * n * n + 9 * n + 2 * ((n + 1) // 2) + (mr + 7) // 8 + 8 + mr * 4 + (mr * 4 + 1) // 2 + 2 * mr + 2 + 64


MR_MAX_64 = max(mr for mr in range(2000) if qp_lds_doubles(64, mr) * 8 <= 160 * 1024)


def spd(rng, n, cond):
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    H = (Q * np.logspace(0, np.log10(cond), n)) @ Q.T
    return 0.5 * (H + H.T)


def rows(rng, n, mr, kind):
    """kind: 'sparse' (1-4 non-zeros per row), 'dense', 'mixed' (half of each)."""
    A = np.zeros((mr, n))
    for r in range(mr):
        if kind == "dense" or (kind == "mixed" and r % 2 == 0):
            A[r] = rng.standard_normal(n)
        else:
            k = int(rng.integers(1, min(4, n) + 1))
            A[r, rng.choice(n, k, replace=False)] = rng.standard_normal(k)
    return A


def problem(rng, n, mr, kind, cond):
    """Feasible QP whose unconstrained minimiser is far outside the polytope: many rows active at the optimum."""
    H = spd(rng, n, cond)
    A = rows(rng, n, mr, kind)
    x0 = rng.integers(-16, 17, n) / 8
    b = A @ x0 + rng.random(mr) * 0.5
    k = min(mr // 10, n // 2)                           # some rows tight at x0 (more than n: test_degenerate_vertices),
    A[:k] = np.round(4 * A[:k]) / 4                     # in quarters and eighths: A x0 is exact, the rows meet at x0
    b[:k] = A[:k] @ x0
    f = -H @ (x0 + 3.0 * rng.standard_normal(n))
    return H, f, A, b


def degenerate(rng, n, kind, cond, extra):
    """n + extra rows tight at a vertex x_v that is the optimum (f = -H x_v - A_t' lam, lam >= 0 on a subset), plus a
    duplicated tight row, an anti-parallel pair pinning x_0 and zero rows."""
    H = spd(rng, n, cond)
    At = np.round(4 * rows(rng, n, n + extra, kind)) / 4       # (quarters and eighths: A_t x_v is exact, the vertex is
    xv = rng.integers(-16, 17, n) / 8                           # not moved by the rounding of b)
    lam = np.where(rng.random(n + extra) < 0.6, rng.random(n + extra) + 0.1, 0.0)
    f = -H @ xv - At.T @ lam
    pin = np.zeros((2, n)); pin[0, 0], pin[1, 0] = 1.0, -1.0
    Ar = rows(rng, n, 20, kind)
    A = np.vstack([At, At[:1], pin, Ar, np.zeros((2, n))])
    b = np.concatenate([At @ xv, At[:1] @ xv, [xv[0], -xv[0]], Ar @ xv + 0.1 + rng.random(20), [0.0, 1.0]])
    act = []                                            # an independent subset of the rows with lam > 0, for kappa
    for i in np.nonzero(lam > 0)[0]:
        if np.linalg.norm(A[i]) > 0 and qr.independent(A, act, int(i)):
            act.append(int(i))
    return H, f, A, b, xv, qr.kkt_kappa(H, A, act)


KIND = {"sparse": 0, "dense": 1, "mixed": 2}


def solve_and_compare(ctx, H, f, A, b, label, worst):
    x, st = ctx.qp_solve(H, f, A, b)
    xo, lam, ok = ko.qp_solve(H, f, A, b)
    assert ok, label
    c = qr.certify_from_oracle(H, f, A, b, lam, xo)
    assert st == 0, label
    err = np.abs(x - c.x).max()
    scale = EPS * c.kappa * max(1.0, np.abs(c.x).max())
    worst[0] = max(worst[0], err / scale)
    print(f"QPMEAS {label} kappa {c.kappa:.4g} xs {np.abs(c.x).max():.3g} err {err:.3g} oracle_err {np.abs(xo - c.x).max():.3g}")
    assert err <= c_tol(c.kappa) * scale, (label, err, c.kappa)
    return c


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("kind", ["sparse", "dense", "mixed"])
def test_sizes_and_row_storage(ctx, n, kind):
    """Each n with 3n rows, the three row stores, cond(H) 1 and 1e4.  Worst C_meas: sparse 2.6e3 (n = 32), dense 5.7e3
    (n = 32), mixed 4.6e3 (n = 63).  (n = 33, sparse, cond 1e4 is test_known_failure_n33_sparse_cond1e4.)"""
    rng = np.random.default_rng(100 * n + KIND[kind])
    worst = [0.0]
    for cond in (1.0, 1e4):
        H, f, A, b = problem(rng, n, 3 * n + 2, kind, cond)
        if (n, kind, cond) == (33, "sparse", 1e4):
            continue                                    # the device fails this one: see the xfail test below
        solve_and_compare(ctx, H, f, A, b, (n, kind, cond), worst)
    print(f"qp_limits sizes n={n} {kind}: worst C_meas {worst[0]:.3g}")


@pytest.mark.parametrize("kind", ["sparse", "dense", "mixed"])
def test_rows_up_to_the_lds_ceiling_at_n64(ctx, kind):
    """n = 64 with MR_MAX_64 (920) rows - the largest count qp_lds_doubles fits in 160 KB - in each row store; then one row
    more is refused.  Worst C_meas: sparse 19, dense 209, mixed 32."""
    assert qp_lds_doubles(64, MR_MAX_64) * 8 <= 160 * 1024 < qp_lds_doubles(64, MR_MAX_64 + 1) * 8
    rng = np.random.default_rng(7 + KIND[kind])
    worst = [0.0]
    H, f, A, b = problem(rng, 64, MR_MAX_64, kind, 1e2)
    c = solve_and_compare(ctx, H, f, A, b, kind, worst)
    assert len(c.active) >= 20                          # a real active set, not the unconstrained minimiser
    A1 = np.vstack([A, A[:1]]); b1 = np.concatenate([b, b[:1]])
    with pytest.raises(F.KoopmanHipError, match="too large"):
        ctx.qp_solve(H, f, A1, b1)
    print(f"qp_limits ceiling {kind}: {len(c.active)} active, worst C_meas {worst[0]:.3g}")


@pytest.mark.parametrize("cond", [1.0, 1e2, 1e4, 1e6, 1e8])
def test_conditioning(ctx, cond):
    """cond(H) 1 ... 1e8 at n = 32 and 64, sparse and dense rows.  Worst C_meas: 0.17 (1), 51 (1e2), 441 (1e4), 1.5e5 (1e6),
    1.2e5 (1e8)."""
    rng = np.random.default_rng(int(np.log10(cond)) + 31)
    worst = [0.0]
    for n in (32, 64):
        for kind in ("sparse", "dense"):
            H, f, A, b = problem(rng, n, 2 * n, kind, cond)
            solve_and_compare(ctx, H, f, A, b, (n, kind), worst)
    print(f"qp_limits cond {cond:g}: worst C_meas {worst[0]:.3g}")


@pytest.mark.parametrize("n", [1, 31, 33, 64])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_degenerate_vertices(ctx, n, kind):
    """More than n rows tight at the optimum, a duplicated tight row, x_0 pinned by an anti-parallel pair, zero rows (one
    with b = 0, one with b = 1).  The optimum is known exactly by construction (the KKT conditions hold at x_v with
    lam >= 0 in exact arithmetic: A_t x_v is exact in quarters and eighths), so x_v is the reference here.
    Worst C_meas: 0.46 (n = 64, dense)."""
    rng = np.random.default_rng(500 + 100 * n + KIND[kind])
    worst = [0.0]
    for cond in (1.0, 1e3):
        H, f, A, b, xv, kappa = degenerate(rng, n, kind, cond, extra=max(1, n // 4))
        assert int((A @ xv == b).sum()) > n + 2
        x, st = ctx.qp_solve(H, f, A, b)
        assert st == 0, (n, kind, cond)
        err = np.abs(x - xv).max()
        scale = EPS * kappa * max(1.0, np.abs(xv).max())
        worst[0] = max(worst[0], err / scale)
        print(f"QPMEAS {(n, kind, cond)} kappa {kappa:.4g} xs {np.abs(xv).max():.3g} err {err:.3g} degenerate")
        assert err <= c_tol(kappa) * scale, (n, kind, cond, err, kappa)
    print(f"qp_limits degenerate n={n} {kind}: worst C_meas {worst[0]:.3g}")


@pytest.mark.xfail(strict=True, reason="kp_qp_solve reports KP_ERR_QP_FAIL on this feasible QP (open)")
def test_known_failure_n33_sparse_cond1e4(ctx):
    """A feasible QP the device solver fails on: n = 33, 101 rows of 1-4 non-zeros (the LDS-copied rows), cond(H) = 1e4,
    31 rows active at the optimum (32 tight), multipliers 19 ... 3.3e4.  The float64 oracle solves it, also with H
    perturbed at 1e-14 and 1e-12, and the reference certifies its optimum; the device returns KP_ERR_QP_FAIL.  Strict: this
    test fails as soon as the solver is fixed, and then moves into test_sizes_and_row_storage."""
    rng = np.random.default_rng(100 * 33 + KIND["sparse"])
    problem(rng, 33, 101, "sparse", 1.0)
    H, f, A, b = problem(rng, 33, 101, "sparse", 1e4)
    solve_and_compare(ctx, H, f, A, b, "n33-sparse-1e4", [0.0])


def simplex_infeasible(rng, kind):
    """n = 64, 900 rows.  Rows 0..63 (a basis: the identity plus 0-3 more non-zeros per row, or dense) with b = B x0 + s,
    row 64 = -(sum of rows 0..63) with b = -(sum of their b) - 1, so rows 0..64 add up to 0 <= -1; 835 slack rows.  A
    minimal infeasible subsystem in 64 variables has at most 65 rows (Caratheodory): here it is rows 0..64, and
    dropping any one of them leaves a feasible problem (checked in the test)."""
    n = 64
    if kind == "sparse":
        B = np.eye(n) + 0.3 * rows(rng, n, n, "sparse") * (rng.random((n, 1)) < 0.75)
        np.fill_diagonal(B, 1.0 + rng.random(n))
    else:
        B = rng.standard_normal((n, n)) + 4 * np.eye(n)
    x0 = rng.standard_normal(n)
    bB = B @ x0 + 0.1 + 0.4 * rng.random(n)
    L = rows(rng, n, 835, kind)
    A = np.vstack([B, -B.sum(axis=0), L])
    b = np.concatenate([bB, [-bB.sum() - 1.0], np.abs(L).sum(axis=1) * 1e3])
    H = spd(rng, n, 10.0)
    f = -H @ (x0 + 3.0 * rng.standard_normal(n))
    return H, f, A, b


def test_infeasible_problems_give_nan_and_qp_fail(ctx):
    """A zero row with b < 0; an anti-parallel pair 1e-6 apart the wrong way; and two 900-row problems at n = 64 whose
    infeasibility needs all 65 rows of a simplex (simplex_infeasible), sparse rows (+ the dense sum row) and dense rows."""
    rng = np.random.default_rng(77)
    cases = []
    H = spd(rng, 5, 10.0); f = rng.standard_normal(5)
    A = rows(rng, 5, 6, "sparse"); b = A @ rng.standard_normal(5) + 1.0
    cases.append((H, f, np.vstack([A, np.zeros((1, 5))]), np.concatenate([b, [-1e-6]])))
    e = np.zeros((2, 5)); e[0, 2], e[1, 2] = 1.0, -1.0
    cases.append((H, f, np.vstack([A, e]), np.concatenate([b, [0.5, -0.5 - 1e-6]])))
    for kind in ("sparse", "dense"):
        H, f, A, b = simplex_infeasible(rng, kind)
        for j in range(65):         # without row j, the 64 other simplex rows hold with equality at x_j, a feasible point
            keep = [i for i in range(65) if i != j]
            xj = np.linalg.solve(A[keep], b[keep])
            assert (np.delete(A, j, 0) @ xj <= np.delete(b, j) + 1e-9 * (1 + np.abs(np.delete(b, j)))).all(), (kind, j)
        cases.append((H, f, A, b))
    for i, (H, f, A, b) in enumerate(cases):
        x, st = ctx.qp_solve(H, f, A, b)
        assert st == F.KP_ERR_QP_FAIL and np.isnan(x).all(), i
        assert not ko.qp_solve(H, f, A, b)[2], i
