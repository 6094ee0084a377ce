"""Test-side reference of the rank-revealing solve (csrc/kp_pivchol.hip: Cholesky with diagonal pivoting of the Gram matrix,
MATLAB's `Px \\ Py` on a rank-deficient dictionary, Ksysid.m:1069): a generator of Gram matrices of KNOWN rank whose
independent columns are known and win every pivot search by a wide margin, an independent left-looking pivoted Cholesky in
np.longdouble with the kernels' stopping rule and tie rule, and the basic solution over a given column subset by QR.  Host
only, numpy only.  Shared by tests/test_pivchol_reference.py (CPU: the reference alone meets the conditions that make the
device comparison unambiguous) and tests/test_gpu_pivchol_regimes.py; not collected by pytest."""
import functools

import numpy as np

EPS = 2.220446049250313e-16

# name -> (W, rank, right-hand sides, seed, duplicate pairs as (index distance, the copy has the LOWER index), expected
# kp_timer_get(17) code = 100 P + 10 S + R, include/koopman_hip.h).  K is the rank-one matrix v v' (make_rank_one).
CASES = {
    "A": (40, 25, 3, 40, (), 111),            # the stop in the middle of the first panel
    "B": (96, 64, 96, 96, (), 111),           # rank a multiple of 32: the stop is found at step 0 of the third panel
    "C": (200, 199, 5, 200, (), 111),         # rank W - 1: only the last pivot is missing
    "D": (200, 120, 5, 201, (), 311),         # under KP_PIVCHOL_GENERIC=1: kp_pivchol_panel_kernel<512, 1>
    "E": (512, 300, 520, 512, (), 121),       # n = 512, 528 padded right-hand sides: kp_trsm2_kernel<4>
    # 16 waves; twins in the same wave, in different waves, and in wave 8 (which exists only in this kernel)
    "F": (530, 400, 7, 530, ((1, False), (64, True), (512, True)), 231),
    "G": (560, 559, 3, 560, (), 231),         # the last W with 32 pivots per panel
    "H": (561, 300, 2, 561, (), 431),         # 31 pivots per panel
    # four rows per thread, 17 pivots per panel; twins in the same thread (other row) and in neighbouring threads
    "I": (1040, 700, 4, 1040, ((1024, True), (1, False)), 531),
    "K": (50, 1, 2, 62, (), 111),             # (seed 50: the largest v^2 is only 1.14 times the second)
}


def _base(W, r, nc, seed):
    rng = np.random.default_rng(seed)
    Ns = 3 * r + 20
    B = rng.standard_normal((Ns, r))
    T = rng.standard_normal((r, W - r)) / np.sqrt(r) * 0.5
    perm = rng.permutation(W)
    P = np.hstack([B, B @ T])[:, perm]
    Y = rng.standard_normal((Ns, nc))
    return P, Y, perm < r


def make_case(W, r, nc, seed, dups=()):
    """P (Ns x W, rank r: r Gaussian columns and W - r combinations of them of about half their norm, shuffled), Y, G = P'P,
    C = P'Y and the sorted indices of the independent columns.  dups: pairs (i, j) - column j, a dependent one, becomes an
    exact copy of the independent column i, in P and bitwise in G (row and column) and C: an exact tie in every pivot search
    until one of the two is chosen.  Of such a pair the independent set holds min(i, j): the lowest index wins a tie."""
    P, Y, ind = _base(W, r, nc, seed)
    for i, j in dups:
        assert ind[i] and not ind[j], (i, j)
        P[:, j] = P[:, i]
    G, C = P.T @ P, P.T @ Y
    for i, j in dups:
        G[j, :] = G[i, :]
        G[:, j] = G[:, i]
        C[j, :] = C[i, :]
        ind[i] = False
        ind[min(i, j)] = True
    return P, Y, G, C, np.flatnonzero(ind)


def pick_dups(W, r, nc, seed, specs):
    """Duplicate pairs (i, j) for make_case out of the case's own permutation: for each (distance, copy_is_lower) the first
    independent column i whose partner j = i -/+ distance is a dependent one (neither used by an earlier pair).  A pair at
    distance 1 lies inside one wave of 64 threads."""
    ind = _base(W, r, 1, seed)[2]
    used, out = set(), []
    for dist, lower in specs:
        for i in np.flatnonzero(ind):
            j = int(i) - dist if lower else int(i) + dist
            if j < 0 or j >= W or ind[j] or i in used or j in used or (dist == 1 and i // 64 != j // 64):
                continue
            out.append((int(i), j))
            used.update((int(i), j))
            break
        else:
            raise AssertionError("no pair at distance %d" % dist)
    return tuple(out)


def make_rank_one(W, nc, seed):
    """G = v v' for a Gaussian v (P = v' is one snapshot): rank 1, the only pivot is argmax v^2."""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((1, W))
    Y = rng.standard_normal((1, nc))
    G, C = P.T @ P, P.T @ Y
    return P, Y, G, C, np.array([int(np.argmax(P[0] ** 2))])


def pivchol_reference(G, rel_tol=None, dependent=()):
    """Left-looking Cholesky with diagonal pivoting in np.longdouble, with the rules csrc/kp_pivchol.hip documents: the pivot
    is the largest remaining diagonal entry, the LOWEST index on ties; it stops at the first pivot pv that misses
    pv > rel_tol d1 (d1 the first pivot; rel_tol = W 64 eps) or pv > 0.  Returns the pivot order, the ratios pv / d1, per
    step the ratio of the chosen pivot to the largest remaining diagonal among the columns `dependent` (inf when none is
    given), and the largest diagonal left at the stop relative to d1."""
    W = G.shape[0]
    if rel_tol is None:
        rel_tol = W * 64 * EPS
    A = G.astype(np.longdouble)
    d = np.diag(A).copy()
    L = np.zeros((W, W), dtype=np.longdouble)         # L[i, k]: column k of the factor
    free = np.ones(W, dtype=bool)
    dep = np.asarray(dependent, dtype=np.int64)
    order, ratios, margins = [], [], []
    d1 = np.longdouble(0)
    for k in range(W):
        p = int(np.argmax(np.where(free, d, -np.inf)))            # the first of equal maxima
        pv = d[p]
        if k == 0:
            d1 = pv
        if not (pv > rel_tol * d1) or not (pv > 0):
            break
        margins.append(float(pv / d[dep].max()) if dep.size and d[dep].max() > 0 else np.inf)
        l = (A[:, p] - L[:, :k] @ L[p, :k]) / np.sqrt(pv)
        l[~free] = 0
        l[p] = np.sqrt(pv)
        L[:, k] = l
        free[p] = False
        d = np.where(free, d - l * l, d)
        order.append(p)
        ratios.append(float(pv / d1))
    left = float(d[free].max() / d1) if free.any() and d1 > 0 else 0.0
    return np.array(order, dtype=np.int64), np.array(ratios), np.array(margins), left


def basic_solution(P, Y, S):
    """Least squares over the columns S of P by Householder QR; the rows outside S are zero."""
    S = np.asarray(S, dtype=np.int64)
    Q, R = np.linalg.qr(P[:, S])
    K = np.zeros((P.shape[1], Y.shape[1]))
    K[S] = np.linalg.solve(R, Q.T @ Y)
    return K


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything the tests share about one case of CASES, computed once: P, Y, G, C, the independent set `ind`, the pairs of
    twins, the reference factorisation (order, ratios, margins, left) and Kref = basic_solution over the reference's set."""
    W, r, nc, seed, specs, code = CASES[name]
    if name == "K":
        dups = ()
        P, Y, G, C, ind = make_rank_one(W, nc, seed)
    else:
        dups = pick_dups(W, r, nc, seed, specs) if specs else ()
        P, Y, G, C, ind = make_case(W, r, nc, seed, dups)
    # the margin is taken over the columns that must never be chosen; the twin with the higher index ties by construction
    dependent = np.setdiff1d(np.arange(W), np.concatenate([ind, np.array([max(p) for p in dups], dtype=np.int64)]))
    order, ratios, margins, left = pivchol_reference(G, dependent=dependent)
    out = dict(W=W, r=r, nc=nc, code=code, P=P, Y=Y, G=G, C=C, ind=ind, dups=dups, order=order, ratios=ratios, margins=margins, left=left,
               Kref=basic_solution(P, Y, np.sort(order)))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
