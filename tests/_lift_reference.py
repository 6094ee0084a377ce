"""Reference of the dictionary lift (kp_lift_kernel, csrc/kp_context.hip) for tests/test_lift_plan.py and
tests/test_gpu_lift_regimes.py.  No device and no library here.

1. `plan`, `fourier_pads`, `fourier_path`: a restatement of the host rules of csrc/kp_lift_plan.h - which launch a batch gets
   (points per workgroup, LDS bytes, descriptors staged or not, the fourier-only loop) and how the digits of a fourier function
   are packed - written from the sizes of the blocks, not from a column list.
2. `lift_full_ld`, `econ_ld`, `rows_ld`: every column straight from its definition (Ksysid.m:484-505 as restated in the docstrings
   of oracle/koopman_oracle.py) in np.longdouble: products, exp, the Hermite recurrence, sin and cos.  The trigonometric ARGUMENT
   is formed in double as 2.0 * pi * j * x, left to right: that rounding belongs to the operation the reference program defines
   (a double times a double), not to the kernel.  The econ layout [v ; pcs' full ; 1] (Ksysid.m:1615-1618) and the rows of Px
   ([psi, u] :1062, [psi, u_1 psi, ...] :1049) are on top of it in long double.
3. `CASES`: the dictionaries and batch sizes of the GPU regime tests with the regime each is named for; the CPU test runs every
   one of them through the plan tool, the GPU test asserts the regime before it lifts.
"""
import math
from dataclasses import dataclass

import numpy as np

from oracle import koopman_oracle as ko

LD = np.longdouble
LDS_BYTES = 160 * 1024
COLDESC_BYTES = 16
FULL, ECON, ROW = 0, 1, 2            # KP_LIFT_FULL / _ECON / _ROW


# ----------------------------------------------------------------------------------------------------------------------
# 1. the host rules
# ----------------------------------------------------------------------------------------------------------------------

def block_sizes(nvars, types, degs):
    """(kind, n) per block as the plan takes them: n = the degree of a fourier block, else the number of functions the block
    adds (poly: the monomials of degree 2..deg, Ksysid.m:488; hermite: all of degree 1..deg; fourier_sparser: those over 2 nvars
    multipliers; gaussian: the centres)."""
    out = []
    for kind, d in zip(types, degs):
        d = int(d)
        if kind == "poly":
            out.append((kind, math.comb(nvars + d, d) - 1 - nvars))
        elif kind == "hermite":
            out.append((kind, math.comb(nvars + d, d) - 1))
        elif kind == "fourier_sparser":
            out.append((kind, math.comb(2 * nvars + d, d) - 1))
        elif kind in ("fourier", "gaussian"):
            out.append((kind, d))
        else:
            raise ValueError(kind)
    return out


def plan(mt, nzeta, m, blocks, k_pcs, rows, num_cu):
    """The launch of kp_lift for `rows` points of the dictionary with these blocks (block_sizes) on a device of num_cu compute
    units: the keys the plan tool prints."""
    nvars = nzeta + (m if mt == "nonlinear" else 0)
    nfull = nvars + 1 + sum((2 * n + 1) ** nvars - 1 if kind == "fourier" else n for kind, n in blocks)
    fdegs = {n for kind, n in blocks if kind == "fourier"}
    # one harmonic table serves the fourier blocks when they share a degree of at most 8
    fdeg = next(iter(fdegs)) if len(fdegs) == 1 and max(fdegs) <= 8 else 0
    # the fourier-only loop: nothing but variables, packed fourier functions (8 nibbles of 0..15) and the constant
    pure = fdeg > 0 and nvars <= 8 and fdeg <= 7 and all(kind == "fourier" or n == 0 for kind, n in blocks)
    doubles = nvars + max(m, 1) + (nvars * (2 * fdeg + 1) if fdeg else 0) + (nfull if k_pcs else 0)
    per_point = 8 * doubles
    threshold = 4 * 64 * (num_cu if num_cu > 0 else 256)
    lt = 64 if 64 * per_point <= LDS_BYTES and rows >= threshold else 16
    out = {"nvars": nvars, "nfull": nfull, "fourier_degree": fdeg, "pure_fourier": pure, "lt": lt}
    if lt * per_point > LDS_BYTES:
        return {**out, "lds": lt * per_point, "stage_cols": 0,
                "error": "kp_lift: dictionary too large for the LDS staging of the pcs projection"}
    staged = lt * per_point + COLDESC_BYTES * nfull <= LDS_BYTES
    return {**out, "lds": lt * per_point + (COLDESC_BYTES * nfull if staged else 0),
            "stage_cols": (1 if staged else 0) | (2 if staged and pure else 0), "error": None}


def fourier_digits(degree, nvars):
    """Digits of fourier functions 1 .. (2 degree + 1)^nvars - 1, one row per function, one column per variable: the position
    of the function in kron(...kron(b(x_0), b(x_1))..., b(x_last)) with b = [1, cos, sin, cos 2, ...] (Ksysid.m:708-724), that is
    the coordinates of a C-ordered grid - the last variable fastest."""
    radix = 2 * degree + 1
    return np.stack(np.unravel_index(np.arange(1, radix ** nvars), (radix,) * nvars), axis=1)


def fourier_pads(degree, nvars):
    """ColDesc::pad of every function of a fourier block: digit of variable v in bits 4 v .. 4 v + 3; zeros when there are
    more than 8 variables or a digit can exceed 15."""
    dg = fourier_digits(degree, nvars)
    if nvars > 8 or 2 * degree > 15:
        return [0] * len(dg)
    return [sum(int(d) << (4 * v) for v, d in enumerate(row)) for row in dg]


def fourier_path(p, mt, blocks, k_pcs, what):
    """Which of the kernel's four fourier evaluations a lift `what` of plan p goes through: 'fourier-only', 'packed table',
    'unpacked table', 'generic'; None for a dictionary without a fourier block."""
    if not any(kind == "fourier" for kind, n in blocks):
        return None
    if p["fourier_degree"] == 0:
        return "generic"
    econ = k_pcs > 0 and what != FULL
    if p["stage_cols"] & 2 and not econ and not (what == ROW and mt == "bilinear"):
        return "fourier-only"
    return "packed table" if p["nvars"] <= 8 and p["fourier_degree"] <= 7 else "unpacked table"


# ----------------------------------------------------------------------------------------------------------------------
# 2. the lift in long double
# ----------------------------------------------------------------------------------------------------------------------

def _harmonic(fn, mult, x):
    """fn(2 pi mult x): the argument in double, left to right, as the reference program forms it; fn in long double."""
    return fn((2.0 * np.pi * float(mult) * x).astype(LD))


def lift_full_ld(basis, V):
    """lift.full of the oracle's Basis on the rows of V (float64), rows x nfull in long double."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    rows, nv = V.shape
    assert nv == basis.nvars
    X = V.astype(LD)
    cols = [X[:, v] for v in range(nv)]                       # Ksysid.m:484
    for kind, arg in basis.blocks:
        if kind == "poly":                                    # prod_v x_v^e_v, without the first nvars rows (:488)
            for e in np.asarray(arg)[nv:]:
                c = np.ones(rows, LD)
                for v in np.nonzero(e)[0]:
                    c = c * X[:, v] ** int(e[v])
                cols.append(c)
        elif kind == "fourier":                               # prod_v b_(digit v)(x_v), without the all-ones product (:724)
            d = int(arg)
            b = np.ones((nv, 2 * d + 1, rows), LD)
            for v in range(nv):
                for j in range(1, d + 1):
                    b[v, 2 * j - 1] = _harmonic(np.cos, j, V[:, v])
                    b[v, 2 * j] = _harmonic(np.sin, j, V[:, v])
            dg = fourier_digits(d, nv)
            c = np.ones((len(dg), rows), LD)
            for v in range(nv):
                c *= b[v][dg[:, v]]
            cols.extend(c)
        elif kind == "gaussian":                              # exp(-|x - c|^2), centres in the columns of arg (:804-806)
            ctr = np.asarray(arg, dtype=np.float64).astype(LD)
            for i in range(ctr.shape[1]):
                r2 = np.zeros(rows, LD)
                for v in range(nv):
                    r2 = r2 + (X[:, v] - ctr[v, i]) ** 2
                cols.append(np.exp(-r2))
        elif kind == "hermite":                               # prod_v H_(n_v)(x_v): H0 = 1, H1 = 2x, H_(k+1) = 2x H_k - 2k H_(k-1)
            for orders in np.asarray(arg):
                c = np.ones(rows, LD)
                for v in np.nonzero(orders)[0]:
                    h0, h1 = np.ones(rows, LD), LD(2) * X[:, v]
                    for k in range(1, int(orders[v])):
                        h0, h1 = h1, LD(2) * X[:, v] * h1 - LD(2 * k) * h0
                    c = c * h1
                cols.append(c)
        elif kind == "fourier_sparser":                       # prod_v sin(2 pi s_v x_v) prod_v cos(2 pi c_v x_v), multipliers [s, c] (:768-786)
            for mult in np.asarray(arg):
                c = np.ones(rows, LD)
                for v in range(nv):
                    if mult[v]:
                        c = c * _harmonic(np.sin, mult[v], V[:, v])
                    if mult[nv + v]:
                        c = c * _harmonic(np.cos, mult[nv + v], V[:, v])
                cols.append(c)
        else:
            raise ValueError(kind)
    cols.append(np.ones(rows, LD))                            # Ksysid.m:505
    return np.stack(cols, axis=1)


def econ_ld(dic, V):
    """lift.econ_full: lift.full, or with a projection [V ; pcs' lift.full(V) ; 1] (Ksysid.m:1615-1618)."""
    full = lift_full_ld(dic.basis, V)
    if dic.pcs is None:
        return full
    X = np.atleast_2d(np.asarray(V, dtype=np.float64)).astype(LD)
    return np.hstack([X, full @ np.asarray(dic.pcs, dtype=np.float64).astype(LD), np.ones((X.shape[0], 1), LD)])


def rows_ld(dic, zeta, u):
    """One row block of Px (Ksysid.m:1034-1064)."""
    zeta = np.atleast_2d(np.asarray(zeta, dtype=np.float64))
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    if dic.model_type == "nonlinear":
        return econ_ld(dic, np.hstack([zeta, u]))
    psi, U = econ_ld(dic, zeta), u.astype(LD)
    if dic.model_type == "bilinear":
        return np.hstack([psi] + [psi * U[:, [i]] for i in range(dic.m)])
    return np.hstack([psi, U])


def solve_ld(A, B):
    """A^-1 B in long double by Gaussian elimination with partial pivoting (numpy's solvers stop at double)."""
    A, B = np.array(A, dtype=LD), np.array(B, dtype=LD)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], B[[k, p]] = A[[p, k]], B[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:] -= f[:, None] * A[k]
        B[k + 1:] -= f[:, None] * B[k]
    for k in range(n - 1, -1, -1):
        B[k] = (B[k] - A[k, k + 1:] @ B[k + 1:]) / A[k, k]
    return B


# ----------------------------------------------------------------------------------------------------------------------
# 3. the cases
# ----------------------------------------------------------------------------------------------------------------------

SMALL = (1, 16, 17, 33)          # one point; exactly one workgroup of 16; one over; two and one


@dataclass(frozen=True)
class Case:
    mt: str
    nz: int
    m: int
    types: tuple
    degs: tuple
    k: int                 # principal axes of a seeded orthonormal projection (0: none)
    rows: tuple            # row counts; "T-1", "T", "T+37" with T = 256 num_cu
    lt: int                # the regime the case is named for: points per workgroup,
    staged: bool           # descriptors in LDS,
    path: tuple            # fourier evaluation of the FULL, ECON and ROW lifts (None: no fourier block)

    @property
    def nvars(self):
        return self.nz + (self.m if self.mt == "nonlinear" else 0)

    @property
    def blocks(self):
        return block_sizes(self.nvars, self.types, self.degs)


def _c(mt, nz, m, types, degs, k=0, rows=SMALL, lt=16, staged=True, path=None):
    return Case(mt, nz, m, tuple(types), tuple(degs), k, tuple(rows), lt, staged, path if isinstance(path, tuple) else (path,) * 3)


FO, PK, UN, GE = "fourier-only", "packed table", "unpacked table", "generic"
FIVE = (["poly", "fourier", "gaussian", "hermite", "fourier_sparser"], [2, 1, 4, 2, 1])
CASES = {
    # A. 64 points per workgroup: T = 256 num_cu rows and more
    "A-linear-poly2-below": _c("linear", 3, 2, ["poly"], [2], rows=["T-1"], lt=16),
    "A-linear-poly2-at": _c("linear", 3, 2, ["poly"], [2], rows=["T"], lt=64),
    "A-linear-poly2-ragged": _c("linear", 3, 2, ["poly"], [2], rows=["T+37"], lt=64),
    "A-bilinear-poly3-pcs": _c("bilinear", 3, 2, ["poly"], [3], k=4, rows=["T+37"], lt=64),
    "A-bilinear-fourier2": _c("bilinear", 2, 2, ["fourier"], [2], rows=["T+37"], lt=64, path=(FO, FO, PK)),
    "A-nonlinear-poly2-gaussian3": _c("nonlinear", 2, 1, ["poly", "gaussian"], [2, 3], rows=["T+37"], lt=64),
    "A-linear10-poly3-pcs": _c("linear", 10, 2, ["poly"], [3], k=4, rows=["T+37"], lt=64),        # 157 152 B of LDS
    "A-linear11-poly3-pcs": _c("linear", 11, 2, ["poly"], [3], k=4, rows=["T+37"], lt=16),        # 64 points would take 193 024 B
    # B. the fourier evaluations
    "B-fourier7-1var": _c("linear", 1, 1, ["fourier"], [7], path=FO),
    "B-fourier1-8vars": _c("linear", 8, 1, ["fourier"], [1], path=FO),                            # 6560 functions, all eight nibbles
    "B-fourier2-2vars": _c("linear", 2, 1, ["fourier"], [2], path=FO),
    "B-fourier1-nonlinear": _c("nonlinear", 2, 1, ["fourier"], [1], path=FO),                     # u is the third variable
    "B-fourier1-twice": _c("linear", 2, 1, ["fourier", "fourier"], [1, 1], path=FO),
    "B-poly2-fourier2-linear": _c("linear", 2, 1, ["poly", "fourier"], [2, 2], path=PK),
    "B-poly2-fourier2-bilinear": _c("bilinear", 2, 1, ["poly", "fourier"], [2, 2], path=PK),
    "B-poly2-fourier2-nonlinear": _c("nonlinear", 2, 1, ["poly", "fourier"], [2, 2], path=PK),
    "B-fourier8-2vars": _c("linear", 2, 1, ["fourier"], [8], path=UN),                            # radix 17
    "B-fourier1-9vars": _c("linear", 9, 1, ["fourier"], [1], rows=[17], staged=False, path=UN),   # 19 682 functions
    "B-fourier9-2vars": _c("linear", 2, 1, ["fourier"], [9], path=GE),
    "B-fourier1-fourier2": _c("linear", 2, 1, ["fourier", "fourier"], [1, 2], path=GE),
    "B-fourier2-pcs": _c("linear", 2, 1, ["fourier"], [2], k=3, path=(FO, PK, PK)),               # the econ path reads the table
    # C. the other block kinds
    "C-five-linear": _c("linear", 3, 1, *FIVE, path=PK),
    "C-five-bilinear": _c("bilinear", 3, 1, *FIVE, path=PK),
    "C-five-nonlinear": _c("nonlinear", 2, 1, *FIVE, path=PK),
    "C-five-linear-pcs": _c("linear", 3, 1, *FIVE, k=5, path=PK),
    "C-five-bilinear-pcs": _c("bilinear", 3, 1, *FIVE, k=5, path=PK),
    "C-five-nonlinear-pcs": _c("nonlinear", 2, 1, *FIVE, k=5, path=PK),
    "C-hermite5-3vars": _c("linear", 3, 1, ["hermite"], [5]),
    "C-fourier_sparser3-2vars": _c("linear", 2, 1, ["fourier_sparser"], [3]),
    "C-poly2-32vars": _c("linear", 32, 1, ["poly"], [2]),                                         # KP_MAX_VARS: exponent bytes not packed
    "C-poly3-9vars": _c("linear", 9, 1, ["poly"], [3]),
}


def row_count(spec, num_cu):
    T = 256 * num_cu
    return {"T-1": T - 1, "T": T, "T+37": T + 37}.get(spec, spec)


def case_dictionary(case, seed=5):
    """The oracle's Dictionary of a case: gaussian centres uniform in [-1, 1] and, with k axes, an orthonormal projection from
    a seeded QR (as test_gram_with_as_many_principal_axes_as_functions makes them)."""
    rng = np.random.default_rng(seed)
    centres = [rng.uniform(-1, 1, (case.nvars, d)) for t, d in zip(case.types, case.degs) if t == "gaussian"]
    dic = ko.build_dictionary(case.mt, case.nz, case.m, list(case.types), list(case.degs), None, False, centres)
    if case.k:
        nfull = dic.basis.nfull
        dic.pcs = np.linalg.qr(np.random.default_rng(case.k).standard_normal((nfull, nfull)))[0][:, :case.k].copy()
    return dic


def case_points(case, rows, seed=3):
    """zeta, u: uniform in [-1, 1] from a fixed seed."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (rows, case.nz)), rng.uniform(-1, 1, (rows, case.m))
