"""Host-side check of the nested sweep's plan (csrc/kp_sweep_plan.h), no device: tools/sweep_plan_check.cpp is built with the
host compiler and run once per dictionary.  The recipes are packed here from exponent rows as kp_basis_create packs them
(byte f of a word = v * Dp + e - 1 for the f-th variable with a non-zero exponent, 255 for none).

What is pinned, for every case of tests/_sweep_reference.py::CASES and the three benchmark shapes (1 variable degree 13 linear,
1 variable degree 6 bilinear, 2 variables degree 4 nonlinear):
  * exponents, degrees, N, W, idx and the column descriptors of every degree;
  * the Chebyshev decision.  The internal basis is Chebyshev exactly when, in every nested dictionary, each product of T_b(x_v)
    (b = a, a - 2, ...) in the expansion of a monomial is itself a column - stated here on the exponent rows.  Every full table
    has that property; so have sparse tables such as B (exponents <= 1: T_1 = x) and C (x^2 beside the constant).  The sparse
    tables G [x, x^9, 1], O, P and Q have not and keep the monomials (Sf = Tinv = I exactly);
  * Sf exactly: products of the coefficients of T_b in x^a, dyadic rationals, from fractions.Fraction - no tolerance;
  * Tinv exactly: the rational inverse of Sf' converted to double, entry for entry - no tolerance (the inverse is integer-valued
    for these tables, largest entry 16640, and the long-double elimination rounds to it without deviation);
  * the four refusals, by their messages;
  * a clean run of the program built with -fsanitize=address,undefined on the benchmark shapes.
"""
import json
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _sweep_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MT = {"linear": 0, "bilinear": 1, "nonlinear": 2}
COL_VAR, COL_MONO, COL_CONST = 0, 1, 4
# name -> (model type, m, nv, exponent rows beyond the variables)
BENCH = {"BENCH_L": ("linear", 1, 1, sr._full(1, 13)), "BENCH_B": ("bilinear", 1, 1, sr._full(1, 6)), "BENCH_N": ("nonlinear", 1, 2, sr._full(2, 4))}


def _shape(name):
    if name in BENCH:
        return BENCH[name]
    mt, n, m, nv, ex, D, N, W, code = sr.case_dims(name)
    return mt, m, nv, ex


def _build(tmp_path_factory, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan_tool") / "sweep_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "koopman-realizations_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "sweep_plan_check.cpp"), "-o", exe]
    return exe, subprocess.run(cmd + extra, capture_output=True, text=True)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe, r = _build(tmp_path_factory, [])
    assert r.returncode == 0, r.stderr
    return exe


def table(nv, ex):
    """All rows of the dictionary: the variables, the monomials, the constant."""
    return np.vstack([np.eye(nv, dtype=np.int64), np.asarray(ex, dtype=np.int64).reshape(-1, nv), np.zeros((1, nv), dtype=np.int64)])


def recipes(rows, Dp):
    words = []
    for row in rows:
        w, f = 0xffffffff, 0
        for v, e in enumerate(row):
            if e:
                w = (w & ~(0xff << (8 * f))) | ((v * Dp + int(e) - 1) << (8 * f))
                f += 1
        words.append(w)
    return words


def run_plan(exe, mt, m, nv, rows, n_deg, Dp=None):
    Dp = Dp or max(1, int(np.max(rows)))
    out = subprocess.run([exe, str(MT[mt]), str(m), str(nv), str(Dp), str(n_deg)] + [str(w) for w in recipes(rows, Dp)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


@pytest.fixture(scope="module")
def plans(tool):
    """The plan of every case at its top degree, computed once."""
    out = {}
    for name in list(sr.CASES) + list(BENCH):
        mt, m, nv, ex = _shape(name)
        rows = table(nv, ex)
        out[name] = run_plan(tool, mt, m, nv, rows, int(rows.sum(axis=1).max()))
    return out


def psi_of_degree(rows, j):
    """Columns of the top dictionary that make the degree-j one: degree <= j, then the constant."""
    deg = rows.sum(axis=1)
    return [c for c in range(len(rows) - 1) if deg[c] <= j] + [len(rows) - 1]


def cheb_coef(a, b):
    """Coefficient of T_b in x^a."""
    if a == 0:
        return Fraction(1 if b == 0 else 0)
    if b > a or (a - b) % 2:
        return Fraction(0)
    c = Fraction(math.comb(a, (a - b) // 2), 2 ** (a - 1))
    return c / 2 if b == 0 else c


def cheb_spans(rows, D):
    """Whether, in every nested dictionary, the Chebyshev products in the expansion of each monomial are columns too."""
    for j in range(1, D + 1):
        have = {tuple(rows[c]) for c in psi_of_degree(rows, j)}
        for c in psi_of_degree(rows, j):
            grids = [range(int(a) % 2, int(a) + 1, 2) for a in rows[c]]
            for b in np.stack(np.meshgrid(*grids, indexing="ij"), -1).reshape(-1, rows.shape[1]):
                if tuple(b) not in have:
                    return False
    return True


def expected_sf(rows, psi, nblk, cheb):
    S = [[Fraction(int(r == c)) for c in range(16)] for r in range(16)]
    Nj = len(psi)
    if cheb:
        for blk in range(nblk):
            for r in range(Nj):
                for c in range(Nj):
                    p = Fraction(1)
                    for a, b in zip(rows[psi[r]], rows[psi[c]]):
                        p *= cheb_coef(int(a), int(b))
                    S[blk * Nj + r][blk * Nj + c] = p
    return S


def exact_inverse(A):
    n = len(A)
    A = [list(r) + [Fraction(int(i == k)) for k in range(n)] for i, r in enumerate(A)]
    for k in range(n):
        p = next(r for r in range(k, n) if A[r][k] != 0)
        A[k], A[p] = A[p], A[k]
        A[k] = [x / A[k][k] for x in A[k]]
        for r in range(n):
            if r != k and A[r][k] != 0:
                A[r] = [x - A[r][k] * y for x, y in zip(A[r], A[k])]
    return [r[n:] for r in A]


ALL = sorted(sr.CASES) + sorted(BENCH)


@pytest.mark.parametrize("name", ALL)
def test_exponents_selection_and_column_descriptors_of_every_degree(plans, name):
    mt, m, nv, ex = _shape(name)
    rows, p = table(nv, ex), plans[name]
    Nmax, D = len(rows), int(rows.sum(axis=1).max())
    assert p["error"] is None and p["dmax"] == D and len(p["degs"]) == D
    assert p["ex"] == rows.tolist() and p["deg"] == rows.sum(axis=1).tolist()
    for j in range(1, D + 1):
        d, psi = p["degs"][j - 1], psi_of_degree(rows, j)
        exj = sr.rows_of_degree(np.asarray(ex).reshape(-1, nv), j)
        assert np.array_equal(rows[psi[nv:-1]], exj) and psi[:nv] == list(range(nv))
        N = nv + exj.shape[0] + 1
        assert (d["N"], d["W"]) == (N, sr.width(mt, m, N))
        if mt == "bilinear":
            idx = [blk * Nmax + c for blk in range(m + 1) for c in psi]
        else:
            idx = psi + ([Nmax + i for i in range(m)] if mt == "linear" else [])
        assert len(idx) == d["W"] and d["idx"] == idx + [0] * (16 - len(idx))
        cols = [[COL_VAR, c] if c < nv else [COL_MONO, c - nv] if c + 1 < Nmax else [COL_CONST, 0] for c in psi]
        assert d["cols"] == cols + [[COL_CONST, 0]] * (16 - N)


@pytest.mark.parametrize("name", ALL)
def test_chebyshev_decision_and_exact_basis_change(plans, name):
    mt, m, nv, ex = _shape(name)
    rows, p = table(nv, ex), plans[name]
    D = int(rows.sum(axis=1).max())
    full = sr.is_full(np.asarray(ex).reshape(-1, nv), nv, D)
    cheb = cheb_spans(rows, D)
    print(name, "full", full, "cheb", p["cheb"])
    assert p["cheb"] == cheb
    if full or name in BENCH:
        assert p["cheb"]
    if name in ("G", "O", "P", "Q"):                  # sparse tables with a Chebyshev term missing; G is the one bb5fe6d fixed
        assert not full and not p["cheb"]
    for j in range(1, D + 1):
        d = p["degs"][j - 1]
        S = expected_sf(rows, psi_of_degree(rows, j), m + 1 if mt == "bilinear" else 1, cheb)
        assert d["Sf"] == [float(x) for r in S for x in r]            # dyadic rationals: exact
        Ti = exact_inverse([[S[c][r] for c in range(16)] for r in range(16)])      # (Sf')^-1
        assert all(x.denominator == 1 and abs(x) <= 16640 for r in Ti for x in r)
        assert d["Tinv"] == [float(x) for r in Ti for x in r]
        if not cheb:
            assert d["Sf"] == d["Tinv"] == [float(r == c) for r in range(16) for c in range(16)]


def test_sets_of_full_and_sparse_cases():
    full = {n for n in sr.CASES if sr.is_full(sr.CASES[n][3], sr.case_dims(n)[3], sr.case_dims(n)[5])}
    assert {"A", "D", "I", "LASSO"} <= full and not full & {"B", "C", "E1", "F", "G", "H", "O", "P", "Q"}


@pytest.mark.parametrize("rows,Dp,n_deg,message", [
    ([[1], [2]], 2, 1, "kp_sweep_eval_nested: the last dictionary column must be the constant"),
    ([[2], [1], [0]], 2, 1, "kp_sweep_eval_nested: monomials must be ordered by total degree"),
    ([[1], [2], [0]], 2, 3, "kp_sweep_eval_nested: n_deg exceeds the degree of the dictionary"),
    ([[3], [3], [0]], 3, 3, "kp_sweep_eval_nested: singular basis change"),       # x^3 twice: T_1 is in neither, S has two equal rows
])
def test_refusals_by_message(tool, rows, Dp, n_deg, message):
    assert run_plan(tool, "linear", 1, 1, np.asarray(rows), n_deg, Dp) == {"error": message}


def test_benchmark_shapes_run_clean_under_address_and_undefined_sanitizers(tmp_path_factory, plans):
    exe, r = _build(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler does not take -fsanitize=address,undefined: " + r.stderr[-200:])
    for name in sorted(BENCH):
        mt, m, nv, ex = _shape(name)
        rows = table(nv, ex)
        assert run_plan(exe, mt, m, nv, rows, int(rows.sum(axis=1).max())) == plans[name]
