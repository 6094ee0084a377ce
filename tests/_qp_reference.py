"""Independent high-precision reference for the dense strictly convex QP  min 1/2 x'Hx + f'x  s.t.  A x <= b.

`certify` does not trust any solver's arithmetic: it takes a candidate active set (the oracle's, or none), solves the
equality-constrained KKT system of that set to ~45 digits (float64 LU with residuals formed in mpmath: mixed-precision
iterative refinement), then runs primal active-set corrections in high precision (add the most violated row, drop the
most negative multiplier) until the point passes the certificate, every test of which is evaluated in mpmath:

    stationarity   |H x + f + A' lam|         <= tol * (1 + |f| + |H| |x|)
    primal         a_i'x - b_i                <= tol * (|a_i| |x| + |b_i| + 1)   for every row
    dual           lam_i                      >= -tol * (1 + |f| + |H| |x|)
    complementary  lam_i (a_i'x - b_i) = 0    (lam is zero off the set, a_i'x = b_i on it to the stationarity accuracy)

with tol = 1e-30.  H is SPD, so x* is unique even at degenerate vertices (more rows tight than variables, duplicated
rows), where lam is not.  The oracle's qp_solve and both device solvers are the same Goldfarb-Idnani iteration with the
same 1e-10 / 1e-13 thresholds; this reference shares neither the algorithm nor the thresholds.

`kappa` is the larger of cond(H) and the 2-norm condition number of the KKT matrix of the final set, [H/|H|  N'; N  0]
with the rows of N normalised: the tests scale their tolerances by it.  (cond(H) enters because every solver here forms
H^-1 explicitly: its error reaches x even where the active rows pin the ill-conditioned directions.)"""
from dataclasses import dataclass

import mpmath
import numpy as np

DPS = 50          # working digits; the certificate holds to 1e-30


class NotCertified(AssertionError):
    pass


@dataclass
class QPCert:
    x: np.ndarray          # float64 rounding of x*
    lam: np.ndarray        # float64 rounding of one multiplier vector (zeros off the active set)
    active: list           # the active set the certificate was built on
    kappa: float           # condition estimate of the KKT matrix of that set
    x_mp: np.ndarray       # x* as mpmath numbers (object array)
    corrections: int       # active-set corrections the candidate needed


def _mp(a):
    return np.vectorize(mpmath.mpf, otypes=[object])(np.asarray(a, dtype=np.float64))


def _kkt_solve(H, Hm, A, Am, f_m, b_m, act):
    """x, lam of  H x + f + N'lam = 0,  N x = b_N  (N = A[act]) to the working precision."""
    n, q = H.shape[0], len(act)
    K = np.zeros((n + q, n + q))
    K[:n, :n] = H
    if q:
        K[:n, n:] = A[act].T
        K[n:, :n] = A[act]
    Km = np.empty((n + q, n + q), dtype=object)
    Km[:n, :n] = Hm
    if q:
        Km[:n, n:] = Am[act].T
        Km[n:, :n] = Am[act]
        Km[n:, n:] = mpmath.mpf(0)
    rhs = np.concatenate([-f_m, b_m[act]]) if q else -f_m.copy()
    z = np.array([mpmath.mpf(0)] * (n + q), dtype=object)
    scale = max(1.0, float(max(abs(v) for v in rhs)))
    goal = mpmath.mpf(10) ** (-(DPS - 8)) * scale
    for _ in range(80):
        res = rhs - Km.dot(z)
        rmax = max(abs(v) for v in res)
        if rmax <= goal:
            return z[:n], z[n:]
        d = np.linalg.solve(K, np.array([float(v) for v in res]))
        if not np.all(np.isfinite(d)):
            break
        z = z + _mp(d)
    raise NotCertified(f"KKT refinement of a {q}-row set did not converge (singular or too ill-conditioned)")


def kkt_kappa(H, A, act):
    """kappa of the module docstring for the active set `act` (independent rows)."""
    n, q = H.shape[0], len(act)
    cH = float(np.linalg.cond(H))
    if q == 0:
        return cH
    N = A[act] / np.linalg.norm(A[act], axis=1, keepdims=True)
    K = np.zeros((n + q, n + q))
    K[:n, :n] = H / np.linalg.norm(H, 2)
    K[:n, n:] = N.T
    K[n:, :n] = N
    return max(cH, float(np.linalg.cond(K)))


def independent(A, act, p):
    """True when row p is linearly independent of the rows in `act` (normalised rows, relative singular value 1e-10)."""
    if len(act) >= A.shape[1]:
        return False
    N = A[act + [p]]
    N = N / np.linalg.norm(N, axis=1, keepdims=True)
    s = np.linalg.svd(N, compute_uv=False)
    return s[-1] > 1e-10 * s[0]


def certify(H, f, A, b, active=None, max_corrections=None):
    """x* and one lam* of the QP, certified to 1e-30 in mpmath at DPS digits.  `active`: candidate active set (row
    indices; the oracle's rows with lam > 0, say), default empty.  Raises NotCertified if no certificate is reached.

    Corrections: while the set's own minimiser is infeasible, the most violated row (by distance) that is independent
    of the set joins it (when there is none, the most negative multiplier leaves; a repeated set ends the attempt).  From
    the first feasible point on, the textbook primal active-set method: drop the most negative multiplier, step toward
    the minimiser of the smaller set and stop at the first blocking row, which joins the set; the objective falls at
    every step, and the point stays feasible."""
    H = np.asarray(H, dtype=np.float64); f = np.asarray(f, dtype=np.float64).ravel()
    A = np.asarray(A, dtype=np.float64).reshape(-1, H.shape[0]); b = np.asarray(b, dtype=np.float64).ravel()
    n, mr = H.shape[0], A.shape[0]
    if max_corrections is None:
        max_corrections = 4 * n + 20
    with mpmath.workdps(DPS):
        tol = mpmath.mpf("1e-30")
        Hm, Am, fm, bm = _mp(H), _mp(A), _mp(f), _mp(b)
        absA, absb = np.abs(A), np.abs(b)
        nrm = np.linalg.norm(A, axis=1)
        act = [int(i) for i in (active if active is not None else [])]
        xf_ = None                    # the current feasible point of the primal phase (None before the first one)
        seen = set()
        for it in range(max_corrections + 1):
            x, lamN = _kkt_solve(H, Hm, A, Am, fm, bm, act)
            xf = np.array([float(v) for v in x])
            xs = max(1.0, float(np.abs(xf).max()))
            dscale = 1.0 + float(np.abs(f).max()) + float(np.abs(H).sum(axis=1).max()) * xs
            slack = (Am.dot(x) - bm) if mr else np.zeros(0, dtype=object)
            pscale = absA.dot(np.abs(xf)) + absb + 1.0
            viol = np.array([float(s / p) for s, p in zip(slack, pscale)]) if mr else np.zeros(0)
            prim_ok = mr == 0 or viol.max() <= float(tol)
            if xf_ is not None and not prim_ok:
                # primal phase: step from the feasible point toward x, blocked by the first row it would cross
                p = x - xf_
                ap = Am.dot(p)
                sl0 = bm - Am.dot(xf_)
                alpha, blk = mpmath.mpf(1), -1
                pn = max(abs(v) for v in p)
                for i in range(mr):      # (rows parallel to the set's see a.p = 0 up to the working precision)
                    if i not in act and ap[i] > mpmath.mpf(10) ** (8 - DPS) * nrm[i] * pn:
                        t = max(sl0[i], mpmath.mpf(0)) / ap[i]
                        if t < alpha:
                            alpha, blk = t, i
                xf_ = xf_ + alpha * p
                if blk < 0 or not independent(A, act, blk):
                    raise NotCertified("primal step blocked by a row dependent on the set")
                act.append(blk)
                continue
            if not prim_ok:
                key = tuple(sorted(act))
                if key in seen:
                    raise NotCertified(f"infeasible-phase corrections cycle at {key}")
                seen.add(key)
                sl = np.array([float(s) for s in slack])
                dist = np.where(nrm > 0, sl / np.where(nrm > 0, nrm, 1.0), np.where(sl > 0, np.inf, -np.inf))
                added = False
                for p_ in np.argsort(-dist):
                    p_ = int(p_)
                    if viol[p_] <= float(tol):
                        break
                    if nrm[p_] == 0:
                        raise NotCertified("a zero row with b < 0: infeasible")
                    if p_ not in act and independent(A, act, p_):
                        act.append(p_); added = True
                        break
                if not added:      # every violated row depends on the set: release the most negative multiplier
                    lm = [float(l) for l in lamN]   # of the rows before the last one added
                    act.pop(int(np.argmin(lm[:-1])) if len(act) > 1 else 0)
                continue
            xf_ = x
            lam_s = np.array([float(l / dscale) for l in lamN])
            stat = Hm.dot(x) + fm + (Am[act].T.dot(lamN) if act else 0)
            if not max(abs(v) for v in stat) <= tol * dscale:
                raise NotCertified("stationarity residual above 1e-30 after refinement")
            if len(act) == 0 or lam_s.min() >= -float(tol):
                lam = np.zeros(mr)
                lam[act] = [float(v) for v in lamN]
                return QPCert(xf, lam, list(act), kkt_kappa(H, A, act), x, it)
            act.pop(int(np.argmin(lam_s)))
        raise NotCertified(f"no certificate after {max_corrections} corrections")


def check_point(H, f, A, b, x, tol=1e-15, active=None):
    """True when x equals the certified optimum to `tol` relative to max(1, |x*|), distance evaluated in mpmath."""
    c = certify(H, f, A, b, active)
    with mpmath.workdps(DPS):
        d = max(abs(mpmath.mpf(float(xi)) - xs) for xi, xs in zip(np.ravel(x), c.x_mp))
        return d <= tol * max(1.0, float(np.abs(c.x).max()))


def oracle_active(lam, A=None, b=None, x=None):
    """Candidate active set from an oracle multiplier vector; with A, b, x also the rows that are tight or violated at x
    within 1e-9 (a float64 solver stops at violations below its 1e-10 threshold), as far as they are independent."""
    act = [int(i) for i in np.nonzero(np.asarray(lam) > 0)[0]]
    if A is None:
        return act
    dist = (A @ x - b) / np.maximum(np.linalg.norm(A, axis=1), 1e-300)
    for i in np.argsort(-dist):
        i = int(i)
        if dist[i] < -1e-9 or len(act) >= A.shape[1]:
            break
        if i not in act and np.linalg.norm(A[i]) > 0 and independent(A, act, i):
            act.append(i)
    return act


def certify_from_oracle(H, f, A, b, lam, x):
    """certify() from the oracle's rows with lam > 0; if that set does not lead to a certificate, from it augmented by the
    rows tight or violated at the oracle's x (see oracle_active)."""
    try:
        return certify(H, f, A, b, oracle_active(lam))
    except NotCertified:
        return certify(H, f, A, b, oracle_active(lam, A, b, x))


def x_error_bound(c: QPCert, C: float):
    """|x - x*|_inf allowed for a float64 solver: C eps kappa max(1, |x*|_inf)."""
    return C * np.finfo(np.float64).eps * c.kappa * max(1.0, float(np.abs(c.x).max()))
