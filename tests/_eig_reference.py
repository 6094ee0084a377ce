"""numpy restatement of kp_eig (csrc/kp_eig_general.hip), step for step: balancing by powers of two without permutation,
Householder reduction to Hessenberg form with Z accumulated forwards, Francis double-shift QR with the kernel's deflation
tests, exceptional shifts and caps, back-substitution on the quasi-triangular T into a separate X, V = Z X, the balancing
undone, unit 2-norm.  The searches that the kernel does as workgroup-wide maximum reductions (the small subdiagonal, the
two consecutive small subdiagonals) are written here as the maximum over the same candidates.  It is the thing to debug on the
CPU; tests/test_eig_reference.py holds it to numpy.linalg.eig with the bounds of the GPU test, and the host tests of
Ksysid.spectrum use it in place of the device.

random_matrix() and fixed_cases() are the matrices that both that test and tests/test_gpu_eig.py run."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
MAX_ITER = 30           # KP_EIG_MAX_ITER
KP_OK, KP_ERR_NOT_CONVERGED = 0, -5
BAL_SWEEPS = 64         # cap of the balancing sweeps (each sweep that changes nothing ends them)


def _cdiv(ar, ai, br, bi):
    s = abs(br) + abs(bi)
    ars, ais, brs, bis = ar / s, ai / s, br / s, bi / s
    s = brs * brs + bis * bis
    return (ars * brs + ais * bis) / s, (ais * brs - ars * bis) / s


def balance(H):
    """In place D^-1 H D, D = diag(scale) of powers of two; returns scale."""
    n = H.shape[0]
    scale = np.ones(n)
    for _ in range(BAL_SWEEPS):
        changed = False
        for i in range(n):
            c = float(np.sum(np.abs(H[:, i])))                 # the diagonal entry counts in both: a row of rounding noise
            r = float(np.sum(np.abs(H[i, :])))                 # beside a diagonal of order one is left alone
            if c == 0.0 or r == 0.0:
                continue
            g, f, s = r / 2.0, 1.0, c + r
            for _k in range(1100):
                if not c < g:
                    break
                f *= 2.0; c *= 4.0
            g = r * 2.0
            for _k in range(1100):
                if not c >= g:
                    break
                f /= 2.0; c /= 4.0
            if (c + r) / f < 0.95 * s:
                scale[i] *= f
                H[i, :] *= 1.0 / f
                H[:, i] *= f
                changed = True
        if not changed:
            break
    return scale


def hessenberg(H, Z):
    """In place Householder reduction; Z (identity on entry, or None) takes the reflectors from the right."""
    n = H.shape[0]
    for m in range(1, n - 1):
        scale = float(np.sum(np.abs(H[m:, m - 1])))
        if scale == 0.0:
            continue
        ort = np.zeros(n)
        ort[m:] = H[m:, m - 1] / scale
        h = float(np.sum(ort[m:] * ort[m:]))
        g = -math.copysign(math.sqrt(h), ort[m])
        h -= ort[m] * g
        ort[m] -= g
        for j in range(m, n):                                   # columns: (I - u u' / h) H
            f = float(np.dot(ort[m:], H[m:, j])) / h
            H[m:, j] -= f * ort[m:]
        for i in range(n):                                      # rows: H (I - u u' / h)
            f = float(np.dot(H[i, m:], ort[m:])) / h
            H[i, m:] -= f * ort[m:]
        if Z is not None:
            for i in range(n):
                f = float(np.dot(Z[i, m:], ort[m:])) / h
                Z[i, m:] -= f * ort[m:]
        H[m, m - 1] = scale * g
        H[m + 1:, m - 1] = 0.0


def hqr(H, Z, wr, wi):
    """Francis double-shift QR on the Hessenberg H, in place.  With Z the reflectors go to the whole of H and to Z, so that H
    ends quasi-triangular; without, to the active window alone.  Returns (iterations, converged, norm)."""
    n = H.shape[0]
    vec = Z is not None
    norm = 0.0
    for j in range(n):
        norm += float(np.sum(np.abs(H[:min(j + 2, n), j])))
    en, its, t, total = n - 1, 0, 0.0, 0
    for _pass in range((MAX_ITER + 1) * n + 1):
        if en < 0:
            break
        l = 0
        for i in range(1, en + 1):                              # the kernel: a maximum reduction over i
            s = abs(H[i - 1, i - 1]) + abs(H[i, i])
            if s == 0.0:
                s = norm
            if s + abs(H[i, i - 1]) == s:
                l = i
        x = H[en, en]
        if l == en:                                             # one root
            wr[en], wi[en] = x + t, 0.0
            H[en, en] = x + t
            en -= 1; its = 0
            continue
        y = H[en - 1, en - 1]
        w = H[en, en - 1] * H[en - 1, en]
        if l == en - 1:                                         # two roots
            p = (y - x) / 2.0
            q = p * p + w
            zz = math.sqrt(abs(q))
            H[en, en] = x + t
            H[en - 1, en - 1] = y + t
            x += t
            if q >= 0.0:                                        # a real pair
                zz = p + math.copysign(zz, p)
                wr[en - 1] = wr[en] = x + zz
                if zz != 0.0:
                    wr[en] = x - w / zz
                wi[en - 1] = wi[en] = 0.0
                if vec:
                    x = H[en, en - 1]
                    s = abs(x) + abs(zz)
                    p, q = x / s, zz / s
                    r = math.sqrt(p * p + q * q)
                    p /= r; q /= r
                    a = H[en - 1, en - 1:].copy(); b = H[en, en - 1:].copy()            # rows
                    H[en - 1, en - 1:] = q * a + p * b
                    H[en, en - 1:] = q * b - p * a
                    a = H[:en + 1, en - 1].copy(); b = H[:en + 1, en].copy()            # columns
                    H[:en + 1, en - 1] = q * a + p * b
                    H[:en + 1, en] = q * b - p * a
                    a = Z[:, en - 1].copy(); b = Z[:, en].copy()
                    Z[:, en - 1] = q * a + p * b
                    Z[:, en] = q * b - p * a
            else:                                               # a complex pair
                wr[en - 1] = wr[en] = x + p
                wi[en - 1], wi[en] = zz, -zz
            en -= 2; its = 0
            continue
        if its == MAX_ITER:
            return total, False, norm
        if its == 10 or its == 20:                              # exceptional shift
            t += x
            for i in range(en + 1):
                H[i, i] -= x
            s = abs(H[en, en - 1]) + abs(H[en - 1, en - 2])
            x = y = 0.75 * s
            w = -0.4375 * s * s
        its += 1; total += 1

        def start(m):
            zz = H[m, m]
            r = x - zz
            s = y - zz
            p = (r * s - w) / H[m + 1, m] + H[m, m + 1]
            q = H[m + 1, m + 1] - zz - r - s
            r = H[m + 2, m + 1]
            s = abs(p) + abs(q) + abs(r)
            return p / s, q / s, r / s
        m = l
        for mm in range(l + 1, en - 1):                         # the kernel: a maximum reduction over mm
            p, q, r = start(mm)
            tst1 = abs(p) * (abs(H[mm - 1, mm - 1]) + abs(H[mm, mm]) + abs(H[mm + 1, mm + 1]))
            tst2 = abs(H[mm, mm - 1]) * (abs(q) + abs(r))
            if tst1 + tst2 == tst1:
                m = mm
        p, q, r = start(m)
        for i in range(m + 2, en + 1):
            H[i, i - 2] = 0.0
            if i != m + 2:
                H[i, i - 3] = 0.0
        for k in range(m, en):                                  # the bulge chase
            notlast = k != en - 1
            if k != m:
                p = H[k, k - 1]
                q = H[k + 1, k - 1]
                r = H[k + 2, k - 1] if notlast else 0.0
                x = abs(p) + abs(q) + abs(r)
                if x == 0.0:
                    continue
                p /= x; q /= x; r /= x
            s = math.copysign(math.sqrt(p * p + q * q + r * r), p)
            if k != m:
                H[k, k - 1] = -s * x
            elif l != m:
                H[k, k - 1] = -H[k, k - 1]
            p += s
            x = p / s; y = q / s; zz = r / s
            q /= p; r /= p
            j1 = n if vec else en + 1
            i0 = 0 if vec else l
            i1 = min(en, k + 3) + 1
            if notlast:
                pp = H[k, k:j1] + q * H[k + 1, k:j1] + r * H[k + 2, k:j1]
                H[k, k:j1] -= pp * x; H[k + 1, k:j1] -= pp * y; H[k + 2, k:j1] -= pp * zz
                pp = x * H[i0:i1, k] + y * H[i0:i1, k + 1] + zz * H[i0:i1, k + 2]
                H[i0:i1, k] -= pp; H[i0:i1, k + 1] -= pp * q; H[i0:i1, k + 2] -= pp * r
                if vec:
                    pp = x * Z[:, k] + y * Z[:, k + 1] + zz * Z[:, k + 2]
                    Z[:, k] -= pp; Z[:, k + 1] -= pp * q; Z[:, k + 2] -= pp * r
            else:
                pp = H[k, k:j1] + q * H[k + 1, k:j1]
                H[k, k:j1] -= pp * x; H[k + 1, k:j1] -= pp * y
                pp = x * H[i0:i1, k] + y * H[i0:i1, k + 1]
                H[i0:i1, k] -= pp; H[i0:i1, k + 1] -= pp * q
                if vec:
                    pp = x * Z[:, k] + y * Z[:, k + 1]
                    Z[:, k] -= pp; Z[:, k + 1] -= pp * q
    return total, True, norm


def _perturb(tst1, v):
    for _k in range(40):
        v *= 0.01
        if not tst1 + v > tst1:
            break
    return v


def backsub(T, wr, wi, norm):
    """X with T X = X diag(lambda) in the packed real form; one column (one pair of columns) per eigenvalue, each independent
    of the others: the kernel gives each to one lane."""
    n = T.shape[0]
    X = np.zeros((n, n))
    if norm == 0.0:
        return np.eye(n)
    for en in range(n):
        p, q = wr[en], wi[en]
        if q == 0.0:                                            # a real vector
            m = en
            X[en, en] = 1.0
            zz = s = 0.0
            for i in range(en - 1, -1, -1):
                w = T[i, i] - p
                r = 0.0
                for j in range(m, en + 1):
                    r += T[i, j] * X[j, en]
                if wi[i] < 0.0:
                    zz, s = w, r
                    continue
                m = i
                if wi[i] == 0.0:
                    t = w
                    if t == 0.0:
                        t = _perturb(norm, norm)
                    X[i, en] = -r / t
                else:
                    x, y = T[i, i + 1], T[i + 1, i]
                    qq = (wr[i] - p) * (wr[i] - p) + wi[i] * wi[i]
                    t = (x * s - zz * r) / qq
                    X[i, en] = t
                    X[i + 1, en] = (-r - w * t) / x if abs(x) > abs(zz) else (-s - y * t) / zz
                t = abs(X[i, en])
                if t != 0.0 and t + 1.0 / t <= t:
                    X[i:en + 1, en] /= t
        elif q < 0.0:                                           # the pair (en - 1, en): real part in en - 1, imaginary in en
            na = en - 1
            m = na
            if abs(T[en, na]) > abs(T[na, en]):
                X[na, na] = q / T[en, na]
                X[na, en] = -(T[en, en] - p) / T[en, na]
            else:
                X[na, na], X[na, en] = _cdiv(0.0, -T[na, en], T[na, na] - p, q)
            X[en, na], X[en, en] = 0.0, 1.0
            zz = r = s = 0.0
            for i in range(en - 2, -1, -1):
                w = T[i, i] - p
                ra = sa = 0.0
                for j in range(m, en + 1):
                    ra += T[i, j] * X[j, na]
                    sa += T[i, j] * X[j, en]
                if wi[i] < 0.0:
                    zz, r, s = w, ra, sa
                    continue
                m = i
                if wi[i] == 0.0:
                    X[i, na], X[i, en] = _cdiv(-ra, -sa, w, q)
                else:
                    x, y = T[i, i + 1], T[i + 1, i]
                    vr = (wr[i] - p) * (wr[i] - p) + wi[i] * wi[i] - q * q
                    vi = (wr[i] - p) * 2.0 * q
                    if vr == 0.0 and vi == 0.0:
                        tst1 = norm * (abs(w) + abs(q) + abs(x) + abs(y) + abs(zz))
                        vr = _perturb(tst1, tst1)
                    X[i, na], X[i, en] = _cdiv(x * r - zz * ra + q * sa, x * s - zz * sa - q * ra, vr, vi)
                    if abs(x) > abs(zz) + abs(q):
                        X[i + 1, na] = (-ra - w * X[i, na] + q * X[i, en]) / x
                        X[i + 1, en] = (-sa - w * X[i, en] - q * X[i, na]) / x
                    else:
                        X[i + 1, na], X[i + 1, en] = _cdiv(-r - y * X[i, na], -s - y * X[i, en], zz, q)
                t = max(abs(X[i, na]), abs(X[i, en]))
                if t != 0.0 and t + 1.0 / t <= t:
                    X[i:en + 1, na] /= t
                    X[i:en + 1, en] /= t
    return X


def eig_general(A, vectors=True):
    """kp_eig of one matrix: (wr, wi, V or None, iters, status), V in the packed real form."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    nan = np.full(n, np.nan)
    if not np.all(np.isfinite(A)):
        return nan, nan.copy(), (np.full((n, n), np.nan) if vectors else None), 0, KP_ERR_NOT_CONVERGED
    H = A.copy()
    scale = balance(H)
    Z = np.eye(n) if vectors else None
    hessenberg(H, Z)
    wr, wi = np.zeros(n), np.zeros(n)
    iters, ok, norm = hqr(H, Z, wr, wi)
    if not ok:
        return nan, nan.copy(), (np.full((n, n), np.nan) if vectors else None), iters, KP_ERR_NOT_CONVERGED
    if not vectors:
        return wr, wi, None, iters, KP_OK
    X = backsub(H, wr, wi, norm)
    V = np.zeros((n, n))
    for j in range(n):
        V[:, j] = Z[:, :j + 1] @ X[:j + 1, j]
    V *= scale[:, None]
    j = 0
    while j < n:
        if wi[j] > 0.0:
            nrm = math.sqrt(float(np.sum(V[:, j] ** 2 + V[:, j + 1] ** 2)))
            V[:, j:j + 2] /= nrm
            j += 2
        else:
            V[:, j] /= math.sqrt(float(np.sum(V[:, j] ** 2)))
            j += 1
    return wr, wi, V, iters, KP_OK


def eig_batch(A, vectors=True):
    """The raw outputs of kp_eig for a stack (nb, n, n): wr, wi (nb, n), V (nb, n, n) or None, iters, status."""
    A = np.asarray(A, dtype=np.float64)
    nb, n = A.shape[0], A.shape[1]
    wr, wi = np.zeros((nb, n)), np.zeros((nb, n))
    V = np.zeros((nb, n, n)) if vectors else None
    iters, status = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    for b in range(nb):
        r = eig_general(A[b], vectors)
        wr[b], wi[b], iters[b], status[b] = r[0], r[1], r[3], r[4]
        if vectors:
            V[b] = r[2]
    return wr, wi, V, iters, status


# ---- what the tests of the restatement and of the device share ------------------------------------------------------------

def complex_vectors(wi, V):
    """The packed real form as complex columns."""
    n = V.shape[0]
    Vc = np.zeros((n, n), dtype=complex)
    j = 0
    while j < n:
        if wi[j] > 0.0:
            Vc[:, j] = V[:, j] + 1j * V[:, j + 1]
            Vc[:, j + 1] = V[:, j] - 1j * V[:, j + 1]
            j += 2
        else:
            Vc[:, j] = V[:, j]
            j += 1
    return Vc


def residual(A, lam, Vc):
    """|| A V - V diag(lam) ||_F / (n eps ||A||_F); 0 for the zero matrix."""
    nA = np.linalg.norm(A)
    if nA == 0.0:
        return float(np.linalg.norm(Vc * lam[None, :]))
    return float(np.linalg.norm(A @ Vc - Vc * lam[None, :]) / (A.shape[0] * EPS * nA))


def random_matrix(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, n))
    if kind == "orth":
        q, r = np.linalg.qr(rng.standard_normal((n, n)))
        return q * np.sign(np.diag(r))[None, :]
    S = rng.standard_normal((n, n))
    S *= 0.8 / np.abs(np.linalg.eigvals(S)).max()
    if kind == "stable":
        return S
    assert kind == "conj", kind
    d = 2.0 ** np.random.default_rng(seed + 1000).integers(-20, 21, n)
    return (S * d[None, :]) / d[:, None]            # inv(D) S D, exact


def cyclic(n):
    return np.roll(np.eye(n), 1, axis=0)


def fixed_cases():
    rng = np.random.default_rng(7)
    hess = np.triu(rng.standard_normal((8, 8)), -1)
    return {
        "real_pair_2": np.array([[2.0, 1.0], [1.0, 3.0]]),
        "complex_pair_2": np.array([[0.5, -2.0], [1.0, 0.5]]),
        "triu_6": np.triu(rng.standard_normal((6, 6))),
        "hessenberg_8": hess,
        "zero_3": np.zeros((3, 3)),
        "identity_4": np.eye(4),
        "cyclic_4": cyclic(4),
        "cyclic_7": cyclic(7),
    }


KINDS = ("gauss", "stable", "orth", "conj")
