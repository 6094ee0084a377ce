"""Thin object wrappers over the C ABI handles (kp_ctx, kp_basis, kp_snapshots, kp_mpc).

Host-side plumbing only: argument marshalling (column-major f64) and handle lifetime.
All arithmetic of the hot path happens inside libkoopman_hip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _ffi as F


def eig_unpack(wr, wi, Vp):
    """The raw outputs of kp_eig, wr / wi (nb, n) and Vp (nb, n, n) with Vp[b][:, j] column j of the packed real form (or
    None), as complex arrays sorted per matrix by decreasing modulus.  The sort is stable on the device's order and ties in
    modulus keep a pair together, the positive imaginary part first."""
    lam = wr + 1j * wi
    V = None
    if Vp is not None:
        V = Vp.astype(complex)
        bs, js = np.nonzero(wi > 0)
        re, im = Vp[bs, :, js], Vp[bs, :, js + 1]
        V[bs, :, js] = re + 1j * im
        V[bs, :, js + 1] = re - 1j * im
    mod = np.abs(lam)
    second = wi < 0                              # the second of a pair takes the modulus of the first: one float, no tie-break by rounding
    mod[second] = np.roll(mod, 1, axis=1)[second]
    order = np.argsort(-mod, axis=1, kind="stable")          # a matrix that failed is all NaN and keeps its order
    lam = np.take_along_axis(lam, order, axis=1)
    if V is not None:
        V = np.take_along_axis(V, order[:, None, :], axis=2)
    return lam, V


class Context:
    """kp_ctx: one per process/GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device_id: int = 0):
        self._h = F.vp()
        F.check(F.lib().kp_create(int(device_id), C.byref(self._h)))
        self.device_id = device_id
        self._children = weakref.WeakSet()       # Basis / Snapshots / Mpc / Traj handles: they hold pointers into this context

    @property
    def handle(self):
        return self._h

    def info(self):
        name = C.create_string_buffer(256)
        ncu = C.c_int()
        hbm = C.c_int64()
        F.check(F.lib().kp_device_info(self._h, name, 256, C.byref(ncu), C.byref(hbm)), self._h)
        return {"name": name.value.decode(), "num_cu": ncu.value, "hbm_bytes": hbm.value}

    def timer(self, which: int) -> float:
        ms = C.c_double()
        F.check(F.lib().kp_timer_get(self._h, which, C.byref(ms)), self._h)
        return ms.value

    def stream(self):
        return F.lib().kp_stream(self._h)

    def synchronize(self):
        """Waits for asynchronous fits (fit(..., fetch=False)); raises if one of them failed."""
        F.check(F.lib().kp_synchronize(self._h), self._h)

    def last_rank(self) -> int:
        """Rank found by the most recent solve (kp_fit_last_rank): W unless the dictionary was rank deficient."""
        r = C.c_int()
        F.check(F.lib().kp_fit_last_rank(self._h, C.byref(r)), self._h)
        return r.value

    def last_pivot_ratio(self) -> float:
        """min_i L_ii^2 / G_ii of the most recent synchronous least-squares solve (~1 / cond(G))."""
        r = C.c_double()
        F.check(F.lib().kp_fit_last_pivot_ratio(self._h, C.byref(r)), self._h)
        return r.value

    def fit_async_slots(self, n_slots: int):
        """Size of the result ring of asynchronous fits (fit(..., fetch=False)): the last n_slots fits of a batch stay
        retrievable with fit_result(q)."""
        F.check(F.lib().kp_fit_async_slots(self._h, int(n_slots)), self._h)

    def fit_result(self, index: int, W: int):
        """K of fit number `index` of the last batch of asynchronous fits (kp_fit_get_K); synchronises."""
        K = np.zeros((W, W), order="F")
        F.check(F.lib().kp_fit_get_K(self._h, int(index), int(W), F.dptr(K)), self._h)
        return K

    def fit_results(self, first: int, count: int, W: int):
        """K of fits first .. first + count - 1 of the last asynchronous batch as one (count, W, W) stack of column-major
        blocks in a page-locked host array of the context ("Kstack": direct DMA, 30 us per 0.9 MB K against 70-260 us
        into pageable memory; valid until the next fit_results call).  K[i].T is fit first + i in numpy's row-major view."""
        out = self.host_array("Kstack", (int(count), W, W))
        for i in range(int(count)):
            F.check(F.lib().kp_fit_get_K(self._h, int(first) + i, int(W), out[i].ctypes.data_as(F.c_dp)), self._h)
        return out

    def host_array(self, name: str, shape):
        """A float64 C-ordered array in page-locked host memory owned by this context (kp_host_alloc), kept under `name`
        and reused by later calls that fit into it: gathers written there cause no page faults and upload by direct DMA.
        The contents belong to the caller until the next host_array(name, ...) call."""
        n = int(np.prod(shape))
        pool = self.__dict__.setdefault("_host_pool", {})
        ent = pool.get(name)
        if ent is None or ent[1] < n:
            if ent is not None:
                F.check(F.lib().kp_host_free(self._h, ent[0]), self._h)
            p = F.vp()
            cap = n + n // 8 + 512
            F.check(F.lib().kp_host_alloc(self._h, cap * 8, C.byref(p)), self._h)
            ent = (p, cap, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(cap,)))
            pool[name] = ent
        return ent[2][:n].reshape(shape)

    def close(self):
        """Destroys the child handles first (their destroy calls dereference the context), then the context."""
        self.__dict__.pop("_host_pool", None)        # the blocks themselves are freed by kp_destroy
        if self._h:
            for ch in list(getattr(self, "_children", ())):
                try:
                    ch.close()
                except Exception:
                    pass
            F.lib().kp_destroy(self._h)
            self._h = F.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stateless entry points ----------------------------------------------------
    def fit_solve(self, G, Cm):
        """K = G \\ C by Cholesky on the device (normal equations of Ksysid.m:1069)."""
        G = F.fcol(G); Cm = F.fcol(Cm)
        W, nc = G.shape[0], Cm.shape[1]
        K = np.zeros((W, nc), order="F")
        F.check(F.lib().kp_fit_solve(self._h, F.dptr(G), F.dptr(Cm), W, nc, F.dptr(K)), self._h)
        return K

    def fit_lasso(self, G, Cm, t, max_iter=20000, tol=1e-10):
        G = F.fcol(G); Cm = F.fcol(Cm)
        W, nc = G.shape[0], Cm.shape[1]
        K = np.zeros((W, nc), order="F")
        it = C.c_int()
        F.check(F.lib().kp_fit_lasso(self._h, F.dptr(G), F.dptr(Cm), W, nc, float(t), int(max_iter), float(tol),
                                     F.dptr(K), C.byref(it)), self._h)
        return K, it.value

    def fit_lasso_batch(self, G, Cm, t, max_iter=20000, tol=1e-10):
        """kp_fit_lasso_batch: all L1 budgets t[v] on the same Grams at once.  Returns ([K_v], iters)."""
        G = F.fcol(G); Cm = F.fcol(Cm)
        W, nc = G.shape[0], Cm.shape[1]
        tv = np.ascontiguousarray(np.atleast_1d(np.asarray(t, dtype=np.float64)))
        K = np.zeros((len(tv), nc, W))                      # each W x nc block column-major
        it = np.zeros(len(tv), dtype=np.int32)
        F.check(F.lib().kp_fit_lasso_batch(self._h, F.dptr(G), F.dptr(Cm), W, nc, F.dptr(tv), len(tv), int(max_iter), float(tol),
                                           F.dptr(K), it.ctypes.data_as(F.c_ip)), self._h)
        return [np.asfortranarray(K[v].T) for v in range(len(tv))], it

    def symm_product(self, G, X, variant=0):
        """kp_symm_product: G X with the product kernels of the lasso iteration alone (G symmetric).  Returns (C, ran):
        ran = F.SYMM_RAN_SMALL, F.SYMM_RAN_NAIVE or F.SYMM_RAN_TILED + 10 RA + RB; an element no lane stored is NaN."""
        G = F.fcol(G); X = F.fcol(X)
        W, nc = X.shape
        if G.shape != (W, W):
            raise ValueError("symm_product: G must be W x W for a W x nc X")
        Cm = np.zeros((W, nc), order="F")
        ran = C.c_int()
        F.check(F.lib().kp_symm_product(self._h, F.dptr(G), F.dptr(X), W, nc, int(variant), F.dptr(Cm), C.byref(ran)), self._h)
        return Cm, ran.value

    def tn_product(self, A, B, Cm, K=None, alpha=1.0, beta=0.0, tri=0, nsplit=1, wa=None, wb=None, form=-1, flags=0):
        """kp_tn_product: Cm = beta Cm + alpha (diag(wa wb) A[:K])' B[:K] with the TN product of the wide path alone.  A (lda, M)
        and B (ldb, N; None with F.TN_SAME) are taken with their leading dimensions as they are, rows K and beyond are padding
        (K defaults to lda); Cm (ldc, N) is a column-major float64 array that is uploaded whole and overwritten IN PLACE with all
        the device buffer holds afterwards, rows beyond M included.  Returns ran = F.TN_RAN_FORM form + F.TN_RAN_VEC vec + the
        splits that ran."""
        A = F.fcol(A)
        B = None if B is None else F.fcol(B)
        if not (isinstance(Cm, np.ndarray) and Cm.dtype == np.float64 and Cm.ndim == 2 and Cm.flags.f_contiguous and Cm.flags.writeable):
            raise ValueError("tn_product: Cm must be a writeable column-major float64 matrix (it is overwritten in place)")
        lda, M = A.shape
        ldb, N = (lda, M) if B is None else B.shape
        if Cm.shape[1] != N:
            raise ValueError("tn_product: Cm must have as many columns as B")
        K = lda if K is None else int(K)
        wa = None if wa is None else np.ascontiguousarray(wa, dtype=np.float64)
        wb = None if wb is None else np.ascontiguousarray(wb, dtype=np.float64)
        if any(w is not None and w.shape != (K,) for w in (wa, wb)):
            raise ValueError("tn_product: wa and wb must have length K")
        ran = C.c_int()
        F.check(F.lib().kp_tn_product(self._h, F.dptr(A), lda, F.dptr(B), ldb, M, N, K, F.dptr(Cm), Cm.shape[0], float(alpha), float(beta),
                                      int(tri), int(nsplit), F.dptr(wa), F.dptr(wb), int(form), int(flags), C.byref(ran)), self._h)
        return ran.value

    def fit_batch(self, basis, snaps, nb):
        """Least-squares fits of nb systems that share one dictionary (W <= 16): `snaps` holds the merged snapshot
        pairs, nb x Ns_each rows.  Returns K, G, C as (nb, W, W) arrays and the status vector."""
        W = basis.W
        Ns_each = snaps.Ns // nb
        K = np.zeros((nb, W, W)); G = np.zeros((nb, W, W)); Cm = np.zeros((nb, W, W))
        st = np.zeros(nb, dtype=np.int32)
        F.check(F.lib().kp_fit_batch(self._h, basis.handle, snaps.handle, nb, Ns_each, F.dptr(K), F.dptr(G), F.dptr(Cm),
                                     st.ctypes.data_as(C.POINTER(C.c_int))), self._h)
        # the library writes column-major W x W blocks: transpose the last two axes of the C-ordered buffers
        return K.transpose(0, 2, 1), G.transpose(0, 2, 1), Cm.transpose(0, 2, 1), st

    def model_project_batch(self, K, G, Cm, N, m):
        """get_model's M-projection (Ksysid.m:1206-1225) for nb small linear models on the device: K, G, Cm (nb, W, W)
        as fit_batch returns them -> A (nb, N, N), B (nb, N, m), status (nb,).  Singular systems give NaN."""
        nb = K.shape[0]
        to_cm = lambda X: np.ascontiguousarray(np.transpose(np.asarray(X, dtype=np.float64), (0, 2, 1)))     # per system column-major
        Kc, Gc, Cc = to_cm(K), to_cm(G), to_cm(Cm)
        A = np.zeros((nb, N, N)); B = np.zeros((nb, max(m, 1), N)); st = np.zeros(nb, dtype=np.int32)
        F.check(F.lib().kp_model_project_batch(self._h, F.dptr(Kc), F.dptr(Gc), F.dptr(Cc), nb, N, m, F.dptr(A), F.dptr(B), None,
                                               st.ctypes.data_as(C.POINTER(C.c_int))), self._h)
        return A.transpose(0, 2, 1), B[:, :m].transpose(0, 2, 1), st

    def sym_eig(self, S):
        """kp_sym_eig: eigenvalues (descending) and eigenvectors (columns) of a symmetric matrix, on the device."""
        S = F.fcol(np.array(S, dtype=np.float64))
        n = S.shape[0]
        V = np.zeros((n, n), order="F"); lam = np.zeros(n); sw = C.c_int()
        F.check(F.lib().kp_sym_eig(self._h, F.dptr(S), n, F.dptr(V), F.dptr(lam), C.byref(sw)), self._h)
        order = np.argsort(-lam, kind="stable")
        return lam[order], np.asfortranarray(V[:, order]), sw.value

    def rollout_nl_batch(self, basis, Kf, zeta0, U):
        """Batched nonlinear rollouts: Kf (nb, nzeta, N), zeta0 (nb, nzeta), U (nb, T, m) -> Z (nb, T, nzeta)."""
        nb, nz, N = Kf.shape
        T = U.shape[1]
        Kf_ = np.ascontiguousarray(np.transpose(Kf, (0, 2, 1)))          # per system column-major nzeta x N
        z0 = np.ascontiguousarray(zeta0, dtype=np.float64)
        U_ = np.ascontiguousarray(np.transpose(U, (0, 2, 1)))            # per system column-major T x m
        Z = np.zeros((nb, nz, T))
        F.check(F.lib().kp_rollout_nl(self._h, basis.handle, nb, F.dptr(Kf_), F.dptr(z0), F.dptr(U_), T, F.dptr(Z)), self._h)
        return np.transpose(Z, (0, 2, 1))

    def model_project(self, K, G, Cm, N, m):
        K = F.fcol(K); G = F.fcol(G); Cm = F.fcol(Cm)
        A = np.zeros((N, N), order="F"); B = np.zeros((N, m), order="F"); M = np.zeros((N, N), order="F")
        F.check(F.lib().kp_model_project(self._h, F.dptr(K), F.dptr(G), F.dptr(Cm), N, m, F.dptr(A), F.dptr(B), F.dptr(M)),
                self._h)
        return A, B, M

    def rollout(self, model_type, A, B, z0, U, n_out):
        """Batched rollouts: A (batch,N,N), B (batch,N,mb), z0 (batch,N), U (batch,T,m) -> Y (batch,T,n_out)."""
        A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
        z0 = np.asarray(z0, dtype=np.float64); U = np.asarray(U, dtype=np.float64)
        single = A.ndim == 2
        if single:
            A, B, z0, U = A[None], B[None], z0[None], U[None]
        batch, N = A.shape[0], A.shape[1]
        T, m = U.shape[1], U.shape[2]
        Ac = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))  # each matrix column-major
        Bc = np.ascontiguousarray(np.transpose(B, (0, 2, 1)))
        Uc = np.ascontiguousarray(np.transpose(U, (0, 2, 1)))
        Y = np.zeros((batch, n_out, T))
        F.check(F.lib().kp_rollout(self._h, F.MODEL[model_type], batch, F.dptr(Ac), F.dptr(Bc), N, m,
                                   F.dptr(np.ascontiguousarray(z0)), F.dptr(Uc), T, n_out, F.dptr(Y)), self._h)
        Y = np.transpose(Y, (0, 2, 1))
        return Y[0] if single else Y

    def rollout_nl(self, basis, Kf, zeta0, U):
        """Nonlinear rollout zeta+ = Kf * econ_full([zeta;u]) on the device: Kf (nzeta,N), zeta0 (nzeta,), U (T,m)
        -> Z (T,nzeta)."""
        Kf = F.fcol(Kf); z0 = np.ascontiguousarray(zeta0, dtype=np.float64); U = F.fcol(np.atleast_2d(U))
        T = U.shape[0]
        Z = np.zeros((T, Kf.shape[0]), order="F")
        F.check(F.lib().kp_rollout_nl(self._h, basis.handle, 1, F.dptr(Kf), F.dptr(z0), F.dptr(U), T, F.dptr(Z)), self._h)
        return Z

    def logm(self, A, shift=0.0, scale=1.0):
        """kp_logm: scale * logm(A_b + shift I) of one n x n matrix or a stack (nb, n, n).  Returns (L, nsqrt, status):
        L NaN and status KP_ERR_NOT_CONVERGED for a matrix without a reachable real principal logarithm."""
        A = np.asarray(A, dtype=np.float64)
        single = A.ndim == 2
        if single:
            A = A[None]
        nb, n = A.shape[0], A.shape[1]
        if A.shape[2] != n:
            raise ValueError("kp_logm: square matrices only")
        Ac = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))        # each matrix column-major
        L = np.zeros_like(Ac)
        nsq = np.zeros(nb, dtype=np.int32); st = np.zeros(nb, dtype=np.int32)
        F.check(F.lib().kp_logm(self._h, nb, n, F.dptr(Ac), float(shift), float(scale), F.dptr(L),
                                nsq.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip)), self._h)
        L = np.transpose(L, (0, 2, 1))
        return (L[0], int(nsq[0]), int(st[0])) if single else (L, nsq, st)

    def eig(self, A, vectors=True):
        """kp_eig: eigenvalues and right eigenvectors of one n x n real matrix or a stack (nb, n, n), one device call.
        Returns (lam, V, iters, status): lam complex, sorted per matrix by decreasing modulus with the positive imaginary part
        of a pair first; V complex with unit columns in that order (None without `vectors`); lam and V NaN and status
        KP_ERR_NOT_CONVERGED for a matrix with a non-finite entry or an eigenvalue that did not deflate."""
        A = np.asarray(A, dtype=np.float64)
        single = A.ndim == 2
        if single:
            A = A[None]
        if A.ndim != 3 or A.shape[2] != A.shape[1]:
            raise ValueError("kp_eig: square matrices only")
        nb, n = A.shape[0], A.shape[1]
        Ac = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))        # each matrix column-major
        wr = np.zeros((nb, n)); wi = np.zeros((nb, n))
        Vp = np.zeros((nb, n, n)) if vectors else None
        it = np.zeros(nb, dtype=np.int32); st = np.zeros(nb, dtype=np.int32)
        F.check(F.lib().kp_eig(self._h, nb, n, F.dptr(Ac), int(bool(vectors)), F.dptr(wr), F.dptr(wi), F.dptr(Vp),
                               it.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip)), self._h)
        lam, V = eig_unpack(wr, wi, None if Vp is None else np.transpose(Vp, (0, 2, 1)))
        if single:
            return lam[0], (None if V is None else V[0]), int(it[0]), int(st[0])
        return lam, V, it, st

    def rollout_ct(self, model_type, A, B, z0, U, n_out, Ts, rtol=1e-3, atol=1e-6):
        """kp_rollout_ct: ode45 over every sample interval of z' = A z + B u (linear) or A z + sum_i u_i B_i z (bilinear),
        batched like `rollout`.  Returns (Y, naccept, nreject, status); a rollout that failed is NaN from the failing
        sample on, with status KP_ERR_NOT_CONVERGED."""
        A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
        z0 = np.asarray(z0, dtype=np.float64); U = np.asarray(U, dtype=np.float64)
        single = A.ndim == 2
        if single:
            A, B, z0, U = A[None], B[None], z0[None], U[None]
        batch, N = A.shape[0], A.shape[1]
        T, m = U.shape[1], U.shape[2]
        Ac = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
        Bc = np.ascontiguousarray(np.transpose(B, (0, 2, 1)))
        Uc = np.ascontiguousarray(np.transpose(U, (0, 2, 1)))
        Y = np.zeros((batch, n_out, T))
        na = np.zeros(batch, dtype=np.int32); nr = np.zeros(batch, dtype=np.int32); st = np.zeros(batch, dtype=np.int32)
        F.check(F.lib().kp_rollout_ct(self._h, F.MODEL[model_type], batch, F.dptr(Ac), F.dptr(Bc), N, m,
                                      F.dptr(np.ascontiguousarray(z0)), F.dptr(Uc), T, n_out, float(Ts), float(rtol), float(atol),
                                      F.dptr(Y), na.ctypes.data_as(F.c_ip), nr.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip)),
                self._h)
        Y = np.transpose(Y, (0, 2, 1))
        return (Y[0], int(na[0]), int(nr[0]), int(st[0])) if single else (Y, na, nr, st)

    def rollout_nl_ct(self, basis, Kf, zeta0, U, Ts, rtol=1e-3, atol=1e-6):
        """kp_rollout_nl_ct: ode45 over every sample interval of zeta' = Kf econ_full([zeta; u]).  Kf (nzeta, N) or
        (nb, nzeta, N), zeta0 (nzeta,) / (nb, nzeta), U (T, m) / (nb, T, m).  Returns (Z, naccept, nreject, status)."""
        Kf = np.asarray(Kf, dtype=np.float64); z0 = np.asarray(zeta0, dtype=np.float64); U = np.asarray(U, dtype=np.float64)
        single = Kf.ndim == 2
        if single:
            Kf, z0, U = Kf[None], z0[None], np.atleast_2d(U)[None]
        nb, nz, N = Kf.shape
        T = U.shape[1]
        Kc = np.ascontiguousarray(np.transpose(Kf, (0, 2, 1)))
        Uc = np.ascontiguousarray(np.transpose(U, (0, 2, 1)))
        Z = np.zeros((nb, nz, T))
        na = np.zeros(nb, dtype=np.int32); nr = np.zeros(nb, dtype=np.int32); st = np.zeros(nb, dtype=np.int32)
        F.check(F.lib().kp_rollout_nl_ct(self._h, basis.handle, nb, F.dptr(Kc), F.dptr(np.ascontiguousarray(z0)), F.dptr(Uc), T,
                                         float(Ts), float(rtol), float(atol), F.dptr(Z), na.ctypes.data_as(F.c_ip),
                                         nr.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip)), self._h)
        Z = np.transpose(Z, (0, 2, 1))
        return (Z[0], int(na[0]), int(nr[0]), int(st[0])) if single else (Z, na, nr, st)

    def arm_simulate(self, params, mode, t, U, W=None, x0=None, Ts=0.0, rtol=1e-3, atol=1e-6):
        """kp_arm_simulate: `batch` arm trials in one launch.  params: the Arm params dict (Nmods, nlinks, l, k, d, m, i, g,
        ku); mode: 'zoh' / 'interp' / 'floor' / 'restart' (include/koopman_hip_arm.h); t (T,) shared by the batch;
        U (batch, T, Nmods); W (batch, T, 2) or None (no load); x0 (batch, 2 Nlinks) or None (rest); Ts: the period of
        'floor'.  Returns (X (batch, T_out, 2 Nlinks), naccept, nreject, status); a failed trial is NaN from its first
        output not reached on, with status KP_ERR_NOT_CONVERGED."""
        p = F.KpArmParams(int(params["Nmods"]), int(params["nlinks"]), *(float(params[f]) for f in ("l", "k", "d", "m", "i", "g", "ku")))
        t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel())
        U = np.ascontiguousarray(np.asarray(U, dtype=np.float64))
        batch, T = U.shape[0], U.shape[1]
        if t.size != T or U.ndim != 3:
            raise ValueError("arm_simulate: U must be (batch, len(t), Nmods)")
        if W is not None:
            W = np.ascontiguousarray(np.broadcast_to(np.asarray(W, dtype=np.float64), (batch, T, 2)))
        if x0 is not None:
            x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(batch, -1))
        n = int(params["Nmods"]) * int(params["nlinks"])
        Tout = T - 1 if mode == "interp" else T
        X = np.zeros((batch, max(Tout, 0), 2 * n))
        na = np.zeros(batch, dtype=np.int32); nr = np.zeros(batch, dtype=np.int32); st = np.zeros(batch, dtype=np.int32)
        F.check(F.lib().kp_arm_simulate(self._h, C.byref(p), F.ARM_MODE[mode], batch, T, F.dptr(t), float(Ts), F.dptr(x0), F.dptr(U),
                                        F.dptr(W), float(rtol), float(atol), F.dptr(X), na.ctypes.data_as(F.c_ip),
                                        nr.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip)), self._h)
        return X, na, nr, st

    def rsys_simulate(self, mode, t, coeffs, pow_x, pow_u, input_gain, x0, U, hold=0, degree_x=None, degree_u=None,
                      rtol=1e-3, atol=1e-6, want_traj=False, want_Y=True):
        """kp_rsys_simulate: nsys x ntrials random-system trials in one launch.  mode: 'span' / 'restart'
        (include/koopman_hip_rsys.h); t (T,); coeffs, pow_x, pow_u (nsys, num_terms); input_gain (nsys,); x0 (ntrials,),
        shared by all systems; U (nsys, ntrials, T) with hold = 0, or the levels (nsys, ntrials, ceil(T / hold)) held
        `hold` samples each.  degree_x / degree_u default to the largest power used.  Returns (Y (nsys, ntrials, T),
        naccept, nreject, status), each (nsys, ntrials) but Y, and with want_traj=True also a finished Traj in the layout
        of Rsys.save_data (the last trial validates) - None when a trial failed (status KP_ERR_NOT_CONVERGED).
        want_Y=False: Y stays on the device (None is returned in its place)."""
        t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel())
        coeffs = np.ascontiguousarray(np.atleast_2d(np.asarray(coeffs, dtype=np.float64)))
        nsys, nterms = coeffs.shape
        px = np.ascontiguousarray(np.asarray(pow_x, dtype=np.int32).reshape(nsys, nterms))
        pu = np.ascontiguousarray(np.asarray(pow_u, dtype=np.int32).reshape(nsys, nterms))
        cu = np.ascontiguousarray(np.asarray(input_gain, dtype=np.float64).reshape(nsys))
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).ravel())
        ntrials, T = x0.size, t.size
        U = np.ascontiguousarray(np.asarray(U, dtype=np.float64))
        width = T if hold == 0 else -(-T // max(int(hold), 1))
        if U.shape != (nsys, ntrials, width):
            raise ValueError(f"rsys_simulate: U must be ({nsys}, {ntrials}, {width})")
        dims = F.KpRsysDims(int(nterms), int(px.max() if degree_x is None else degree_x), int(pu.max() if degree_u is None else degree_u))
        Y = np.zeros((nsys, ntrials, T)) if want_Y else None
        na = np.zeros((nsys, ntrials), dtype=np.int32); nr = np.zeros_like(na); st = np.zeros_like(na)
        h = F.vp()
        rc = F.lib().kp_rsys_simulate(self._h, C.byref(dims), F.RSYS_MODE[mode], nsys, ntrials, T, F.dptr(t), F.dptr(coeffs),
                                      px.ctypes.data_as(F.c_ip), pu.ctypes.data_as(F.c_ip), F.dptr(cu), F.dptr(x0), F.dptr(U),
                                      int(hold), float(rtol), float(atol), F.dptr(Y), na.ctypes.data_as(F.c_ip),
                                      nr.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip), C.byref(h) if want_traj else None)
        if not want_traj:
            F.check(rc, self._h)
            return Y, na, nr, st
        if rc == F.KP_ERR_NOT_CONVERGED:           # some trial failed: its status says which, and there is no object
            return Y, na, nr, st, None
        F.check(rc, self._h)
        return Y, na, nr, st, Traj.from_handle(self, h)

    def lift_jacobian(self, basis, V):
        """kp_lift_jacobian: d econ_full / dv at the rows of V (rows x nvars; v = [zeta, u] for a nonlinear dictionary)
        -> (rows, N, nvars)."""
        V = F.fcol(np.atleast_2d(V))
        rows = V.shape[0]
        J = np.zeros((rows, basis.nvars, basis.N))          # per row an N x nvars column-major block
        F.check(F.lib().kp_lift_jacobian(self._h, basis.handle, rows, F.dptr(V), F.dptr(J)), self._h)
        return np.transpose(J, (0, 2, 1))

    def load_observe(self, basis, model_type, A, B, nw, trials, win_trial, win_start, hor, whatpast=None, flags=0):
        """kp_load_observe: the load estimate of every window, one call.  basis: the unloaded dictionary; A, B: the loaded
        model (N (nw + 1) rows); trials: a list of (zeta, u) pairs of row arrays (rows x nzeta, rows x m), already padded;
        window w covers rows win_start[w] .. win_start[w] + hor - 1 of trial win_trial[w].  whatpast (nwin x nw) with
        flags & OBS_RATE.  Returns (what (nwin x nw), resnorm (nwin), status (nwin)): NaN and KP_ERR_QP_FAIL for a window
        without a unique estimate."""
        zs = [np.asarray(z, dtype=np.float64).reshape(-1, basis.nzeta) for z, _ in trials]
        us = [np.asarray(u, dtype=np.float64).reshape(-1, basis.m) for _, u in trials]
        if any(z.shape[0] != u.shape[0] for z, u in zip(zs, us)):
            raise ValueError("every trial needs as many input rows as state rows")
        lens = [z.shape[0] for z in zs]
        Z = F.fcol(np.vstack(zs)); U = F.fcol(np.vstack(us)); A = F.fcol(A); B = F.fcol(B)
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)]), dtype=np.int64)
        wt = np.ascontiguousarray(win_trial, dtype=np.int32); ws = np.ascontiguousarray(win_start, dtype=np.int64)
        nwin = wt.size
        if ws.size != nwin:
            raise ValueError("win_trial and win_start must have the same length")
        wp = None if whatpast is None else np.ascontiguousarray(np.asarray(whatpast, dtype=np.float64).reshape(nwin, int(nw)))
        what = np.zeros((nwin, int(nw))); res = np.zeros(nwin); st = np.zeros(nwin, dtype=np.int32)
        F.check(F.lib().kp_load_observe(self._h, basis.handle, F.MODEL[model_type], F.dptr(A), F.dptr(B), int(nw), int(Z.shape[0]),
                                        F.dptr(Z), F.dptr(U), len(trials), off.ctypes.data_as(C.POINTER(C.c_int64)), nwin,
                                        wt.ctypes.data_as(C.POINTER(C.c_int32)), ws.ctypes.data_as(C.POINTER(C.c_int64)),
                                        int(hor), F.dptr(wp), int(flags), F.dptr(what), F.dptr(res),
                                        st.ctypes.data_as(F.c_ip)), self._h)
        return what, res, st

    @staticmethod
    def _validate_pack(basis, model_type, models, trials, n, nw):
        """The arguments of kp_validate / kp_validate_ct: (A, B, off, z0, U, Y, W) in the layouts of the header."""
        N, m, nz = basis.N, basis.m, basis.nzeta
        NL = N * (nw + 1)
        if model_type == "nonlinear":
            A = np.ascontiguousarray(np.stack([np.asarray(k, dtype=np.float64).reshape(nz, NL).T for k in models]))
            B = None
        else:
            mb = m * NL if model_type == "bilinear" else m
            A = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float64).reshape(NL, NL).T for a, _ in models]))
            B = np.ascontiguousarray(np.stack([np.asarray(b, dtype=np.float64).reshape(NL, mb).T for _, b in models]))
        Us = [np.asarray(u, dtype=np.float64).reshape(-1, m) for _, u, _, _ in trials]
        Ys = [np.asarray(y, dtype=np.float64).reshape(-1, n) for _, _, y, _ in trials]
        lens = [y.shape[0] for y in Ys]
        if any(u.shape[0] != T for u, T in zip(Us, lens)):
            raise ValueError("every trial needs as many input rows as output rows")
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)]), dtype=np.int64)
        z0 = F.fcol(np.stack([np.asarray(z, dtype=np.float64).reshape(nz) for z, _, _, _ in trials]))
        U = F.fcol(np.vstack(Us)); Y = F.fcol(np.vstack(Ys))
        W = None
        if nw > 0:
            Ws = [np.asarray(w, dtype=np.float64).reshape(-1, nw) for _, _, _, w in trials]
            if any(w.shape[0] != T for w, T in zip(Ws, lens)):
                raise ValueError("every trial needs as many load rows as output rows")
            W = F.fcol(np.vstack(Ws))
        return A, B, off, z0, U, Y, W

    def validate(self, basis, model_type, models, trials, n, nw, yfactor, want_sim=False):
        """kp_validate: every model rolled out over every trial in one launch, the errors of get_error reduced on the device.
        basis: the unloaded dictionary; models: a list of (A, B) (linear, bilinear; loaded models at their full width
        N (nw + 1)) or of Kf (nonlinear); trials: a list of (zeta0 (nzeta), U (T x m), Yreal (T x n), Wl (T x nw) or None),
        the rows after the nd shift; yfactor (n): the factors of scaleup.y.  Returns (err (nmod, ntr, 3 n + 2):
        [mean | rmse | nrmse | euclid_mean | unscaled euclid_mean], status (nmod, ntr): 1 where the simulated outputs left
        the finite range, sim: a list per model of a list per trial of T x n arrays, or None)."""
        N, m, nz, n, nw = basis.N, basis.m, basis.nzeta, int(n), int(nw)
        nmod, ntr = len(models), len(trials)
        A, B, off, z0, U, Y, W = self._validate_pack(basis, model_type, models, trials, n, nw)
        rows = int(off[-1])
        fac = np.ascontiguousarray(np.broadcast_to(np.asarray(yfactor, dtype=np.float64), (n,)))
        err = np.zeros((nmod, ntr, 3 * n + 2)); st = np.zeros((nmod, ntr), dtype=np.int32)
        S = np.zeros((nmod, n, rows)) if want_sim else None
        F.check(F.lib().kp_validate(self._h, basis.handle, F.MODEL[model_type], N, m, n, nz, nw, nmod, F.dptr(A), F.dptr(B), ntr,
                                    off.ctypes.data_as(C.POINTER(C.c_int64)), F.dptr(z0), F.dptr(U), F.dptr(Y), F.dptr(W),
                                    F.dptr(fac), int(bool(want_sim)), F.dptr(err), st.ctypes.data_as(F.c_ip), F.dptr(S)), self._h)
        sim = None
        if want_sim:
            sim = [[np.ascontiguousarray(S[i, :, off[q]:off[q + 1]].T) for q in range(ntr)] for i in range(nmod)]
        return err, st, sim

    def validate_horizon(self, basis, model_type, models, trials, n, yfactor, horizon, stride=1):
        """kp_validate_horizon: the h-step-ahead prediction errors, h = 1 .. horizon, of every model from every start sample
        of every trial, one device call.  basis: the unloaded dictionary; models as `validate` takes them (nw = 0); trials: a
        list of (Zeta (T x nzeta), U (T x m)), the delay-embedded states and inputs after the nd shift - the first n columns
        of Zeta are the real outputs; starts s = 0, stride, ... while s + horizon <= T - 1.  Returns (err (nmod, ntr, horizon,
        2 n + 2): [mean |d| | rmse | euclid_mean | unscaled euclid_mean] over the starts of the trial, NaN for a trial without
        a start; starts (ntr); status (nmod, ntr): 1 where a prediction left the finite range)."""
        N, m, nz, n = basis.N, basis.m, basis.nzeta, int(n)
        nmod, ntr, H = len(models), len(trials), int(horizon)
        Zs = [np.asarray(z, dtype=np.float64).reshape(-1, nz) for z, _ in trials]
        packed = [(z[0] if z.shape[0] else np.zeros(nz), u, z[:, :min(n, nz)], None) for z, (_, u) in zip(Zs, trials)]
        A, B, off, _, U, _, _ = self._validate_pack(basis, model_type, models, packed, min(n, nz), 0)
        Z = F.fcol(np.vstack(Zs))
        fac = np.ascontiguousarray(np.broadcast_to(np.asarray(yfactor, dtype=np.float64), (n,)))
        err = np.zeros((nmod, ntr, max(H, 0), 2 * n + 2)); st = np.zeros((nmod, ntr), dtype=np.int32)
        ns = np.zeros(ntr, dtype=np.int64)
        F.check(F.lib().kp_validate_horizon(self._h, basis.handle, F.MODEL[model_type], N, m, n, nz, nmod, F.dptr(A), F.dptr(B), ntr,
                                            off.ctypes.data_as(C.POINTER(C.c_int64)), F.dptr(Z), F.dptr(U), F.dptr(fac), H,
                                            int(stride), F.dptr(err), ns.ctypes.data_as(C.POINTER(C.c_int64)),
                                            st.ctypes.data_as(F.c_ip)), self._h)
        return err, ns, st

    def validate_ct(self, basis, model_type, models, trials, n, yfactor, Ts, rtol=1e-3, atol=1e-6, want_sim=False, nw=0):
        """kp_validate_ct: `validate` for continuous-time models - every sample interval of every (model, trial) pair is ode45
        over [0, Ts] with the input held (the step control of rollout_ct / rollout_nl_ct), one launch for the whole table.
        models and trials as `validate` takes them (no loads: the fourth entry of a trial is ignored, and nw other than 0 is
        refused by the library).  Returns (err, status, sim, naccept, nreject): err, status and sim as `validate`, status 1
        also where the integration failed (the samples from the failing one on are NaN); naccept, nreject (nmod, ntr): the
        accepted / rejected steps of each pair."""
        N, m, nz, n, nw = basis.N, basis.m, basis.nzeta, int(n), int(nw)
        nmod, ntr = len(models), len(trials)
        A, B, off, z0, U, Y, _ = self._validate_pack(basis, model_type, models, trials, n, 0)
        rows = int(off[-1])
        fac = np.ascontiguousarray(np.broadcast_to(np.asarray(yfactor, dtype=np.float64), (n,)))
        err = np.zeros((nmod, ntr, 3 * n + 2)); st = np.zeros((nmod, ntr), dtype=np.int32)
        na = np.zeros((nmod, ntr), dtype=np.int32); nr = np.zeros((nmod, ntr), dtype=np.int32)
        S = np.zeros((nmod, n, rows)) if want_sim else None
        F.check(F.lib().kp_validate_ct(self._h, basis.handle, F.MODEL[model_type], N, m, n, nz, nw, nmod, F.dptr(A), F.dptr(B), ntr,
                                       off.ctypes.data_as(C.POINTER(C.c_int64)), F.dptr(z0), F.dptr(U), F.dptr(Y), None,
                                       F.dptr(fac), int(bool(want_sim)), float(Ts), float(rtol), float(atol), F.dptr(err),
                                       st.ctypes.data_as(F.c_ip), F.dptr(S), na.ctypes.data_as(F.c_ip), nr.ctypes.data_as(F.c_ip)),
                self._h)
        sim = None
        if want_sim:
            sim = [[np.ascontiguousarray(S[i, :, off[q]:off[q + 1]].T) for q in range(ntr)] for i in range(nmod)]
        return err, st, sim, na, nr

    def qp_solve(self, H, f, A, b):
        """quadprog_gurobi(H,f,A,b) shim: NaN vector on failure (quadprog_gurobi.m:22-23)."""
        H = F.fcol(H); A = F.fcol(A)
        f = np.ascontiguousarray(f, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
        n, mr = H.shape[0], A.shape[0]
        x = np.zeros(n)
        st = C.c_int()
        F.check(F.lib().kp_qp_solve(self._h, F.dptr(H), F.dptr(f), F.dptr(A), F.dptr(b), n, mr, F.dptr(x), C.byref(st)),
                self._h)
        return x, st.value


def basis_desc(model_type, nzeta, m, blocks, pcs=None):
    """kp_basis_desc of a host-side dictionary description (blocks as Basis takes them).  Returns (desc, keep): `keep`
    holds the arrays the descriptor points into and must outlive every call that is handed the descriptor."""
    nvars = nzeta + (m if model_type == "nonlinear" else 0)
    btype, bcount, exps, centres = [], [], [], []
    for kind, arg in blocks:
        btype.append(F.BLOCK[kind])
        if kind in ("poly", "hermite"):
            e = np.ascontiguousarray(arg, dtype=np.uint8).reshape(-1, nvars)
            bcount.append(e.shape[0]); exps.append(e)
        elif kind == "fourier_sparser":
            e = np.ascontiguousarray(arg, dtype=np.uint8).reshape(-1, 2 * nvars)
            bcount.append(e.shape[0]); exps.append(e.reshape(-1, nvars))      # two table rows per function
        elif kind == "fourier":
            bcount.append(int(arg))
        else:
            c = np.asarray(arg, dtype=np.float64).reshape(nvars, -1)
            bcount.append(c.shape[1]); centres.append(np.ascontiguousarray(c.T))  # centre-major
    bt = np.array(btype, dtype=np.int32); bc = np.array(bcount, dtype=np.int32)
    ex = np.ascontiguousarray(np.vstack(exps)) if exps else np.zeros((0, nvars), np.uint8)
    ce = np.ascontiguousarray(np.vstack(centres)) if centres else np.zeros((0, nvars))
    pc = None if pcs is None else F.fcol(pcs)
    d = F.KpBasisDesc()
    d.model_type, d.nzeta, d.m, d.n_blocks = F.MODEL[model_type], nzeta, m, len(blocks)
    d.block_type = bt.ctypes.data_as(C.POINTER(C.c_int32))
    d.block_count = bc.ctypes.data_as(C.POINTER(C.c_int32))
    d.poly_exps = ex.ctypes.data_as(C.POINTER(C.c_uint8))
    d.gauss_centres = F.dptr(ce)
    d.k_pcs = 0 if pcs is None else pc.shape[1]
    d.pcs = F.dptr(pc)
    return d, (bt, bc, ex, ce, pc)


class Basis:
    """kp_basis built from a host-side dictionary description (see basis.py)."""

    def __init__(self, ctx: Context, model_type, nzeta, m, blocks, pcs=None):
        """blocks: list of ('poly', exps[rows,nvars] uint8) | ('fourier', deg) | ('gaussian', centres[nvars,k])
        | ('hermite', orders[rows,nvars] uint8) | ('fourier_sparser', multipliers[rows,2*nvars] uint8)."""
        self.ctx = ctx
        ctx._children.add(self)
        d, self._keep = basis_desc(model_type, nzeta, m, blocks, pcs)
        self._h = F.vp()
        F.check(F.lib().kp_basis_create(ctx.handle, C.byref(d), C.byref(self._h)), ctx.handle)
        nv, nf, N, W = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        F.check(F.lib().kp_basis_dims(self._h, C.byref(nv), C.byref(nf), C.byref(N), C.byref(W)))
        self.nvars, self.nfull, self.N, self.W = nv.value, nf.value, N.value, W.value
        self.model_type, self.nzeta, self.m = model_type, nzeta, m

    @property
    def handle(self):
        return self._h

    def lift(self, what, zeta, u=None):
        zeta = F.fcol(np.atleast_2d(zeta))
        rows = zeta.shape[0]
        uu = None if u is None else F.fcol(np.atleast_2d(u))
        width = {F.LIFT_FULL: self.nfull, F.LIFT_ECON: self.N, F.LIFT_ROW: self.W}[what]
        out = np.zeros((rows, width), order="F")
        F.check(F.lib().kp_lift(self.ctx.handle, self._h, what, F.dptr(zeta), F.dptr(uu), rows, F.dptr(out)),
                self.ctx.handle)
        return out

    def close(self):
        if self._h:
            F.lib().kp_basis_destroy(self._h)
            self._h = F.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Snapshots:
    """kp_snapshots: snapshot pairs resident in HBM."""

    def __init__(self, ctx: Context, alpha, beta, u):
        self.ctx = ctx
        ctx._children.add(self)
        a = F.fcol(alpha); b = F.fcol(beta); uu = F.fcol(u)
        self.Ns, self.nzeta, self.m = a.shape[0], a.shape[1], uu.shape[1]
        self._h = F.vp()
        F.check(F.lib().kp_snapshots_upload(ctx.handle, F.dptr(a), F.dptr(b), F.dptr(uu), self.Ns, self.nzeta, self.m,
                                            C.byref(self._h)), ctx.handle)

    def update(self, alpha, beta, u):
        """kp_snapshots_update: new pairs into the same device arrays.  Returns once the host arrays are staged; the
        transfer overlaps whatever the device is doing with OTHER snapshot objects (keep two and alternate)."""
        a = F.fcol(alpha); b = F.fcol(beta); uu = F.fcol(u)
        if a.shape[1] != self.nzeta or uu.shape[1] != self.m or b.shape != a.shape or uu.shape[0] != a.shape[0]:
            raise ValueError("Snapshots.update: column counts must match the object")
        F.check(F.lib().kp_snapshots_update(self.ctx.handle, self._h, F.dptr(a), F.dptr(b), F.dptr(uu), a.shape[0]), self.ctx.handle)
        self.Ns = a.shape[0]
        return self

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            F.lib().kp_snapshots_destroy(self._h)
            self._h = F.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Traj:
    """kp_traj: training / validation trajectories of nb systems with one layout, resident on the device (raw values;
    the per-system scaling of get_scale is computed there).  Y (nb, rows, n), U (nb, rows, m) with rows = ntrials * T
    (merged trials), Yv (nb, Tv, n), Uv (nb, Tv, m)."""

    def __init__(self, ctx: Context, Y, U, ntrials, Yv, Uv):
        self.ctx = ctx
        ctx._children.add(self)
        Y = np.asarray(Y, dtype=np.float64); U = np.asarray(U, dtype=np.float64)
        Yv = np.asarray(Yv, dtype=np.float64); Uv = np.asarray(Uv, dtype=np.float64)
        self.nb, rows, self.n = Y.shape
        self.m = U.shape[2]
        self.ntrials, self.T, self.Tv = int(ntrials), rows // int(ntrials), Yv.shape[1]
        if self.T * self.ntrials != rows:
            raise ValueError("Traj: rows must be ntrials * T")
        tr = Traj._blocks
        self._h = F.vp()
        F.check(F.lib().kp_traj_upload(ctx.handle, F.dptr(tr(Y)), F.dptr(tr(U)), self.nb, self.ntrials, self.T, self.n, self.m,
                                       F.dptr(tr(Yv)), F.dptr(tr(Uv)), self.Tv, C.byref(self._h)), ctx.handle)

    @staticmethod
    def _blocks(a):
        """(nb, rows, width) -> each system column-major rows x width (no copy for width 1)."""
        return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))

    @classmethod
    def begin(cls, ctx: Context, nb, ntrials, T, n, m, Tv):
        """kp_traj_create: the object in three steps (begin, put x 4, finish), so that a caller that assembles the blocks one
        after the other has each on its way to the device while it prepares the next."""
        self = cls.__new__(cls)
        self.ctx = ctx
        ctx._children.add(self)
        self.nb, self.ntrials, self.T, self.n, self.m, self.Tv = int(nb), int(ntrials), int(T), int(n), int(m), int(Tv)
        self._h = F.vp()
        self._keep = []
        F.check(F.lib().kp_traj_create(ctx.handle, self.nb, self.ntrials, self.T, self.n, self.m, self.Tv, C.byref(self._h)), ctx.handle)
        return self

    @classmethod
    def from_handle(cls, ctx: Context, h):
        """Wrap an existing, finished kp_traj handle (made on the device, e.g. by kp_rsys_simulate); the object owns it from
        now on.  The layout is read back with kp_traj_dims."""
        self = cls.__new__(cls)
        self.ctx = ctx
        ctx._children.add(self)
        self._h = h if isinstance(h, F.vp) else F.vp(h)
        self._keep = []
        d = [C.c_int() for _ in range(6)]
        F.check(F.lib().kp_traj_dims(self._h, *(C.byref(v) for v in d)), ctx.handle)
        self.nb, self.ntrials, self.T, self.n, self.m, self.Tv = (v.value for v in d)
        return self

    def put(self, which, a):
        """kp_traj_put: block 'Y' | 'U' | 'Yv' | 'Uv' as (nb, rows, width); asynchronous when `a` lies in page-locked memory
        (Context.host_array), which must stay untouched until finish()."""
        w = {"Y": 0, "U": 1, "Yv": 2, "Uv": 3}[which]
        a = np.asarray(a, dtype=np.float64)
        want = (self.nb, (self.ntrials * self.T) if w < 2 else self.Tv, self.n if w in (0, 2) else self.m)
        if a.shape != want:
            raise ValueError(f"Traj.put: block {which} has shape {a.shape}, expected {want}")
        blk = Traj._blocks(a)
        self._keep.append(blk)                                                # alive until the copy has been waited for
        F.check(F.lib().kp_traj_put(self._h, w, F.dptr(blk)), self.ctx.handle)

    def finish(self):
        """kp_traj_finish: scaling on the device, stream synchronised - the object is ready."""
        F.check(F.lib().kp_traj_finish(self._h), self.ctx.handle)
        self._keep = []
        return self

    @property
    def handle(self):
        return self._h

    def scale(self):
        """Per system [y offset (n) | y factor (n) | u offset (m) | u factor (m)] as computed on the device."""
        sc = np.zeros((self.nb, 2 * (self.n + self.m)))
        F.check(F.lib().kp_traj_scale(self._h, F.dptr(sc)), self.ctx.handle)
        return sc

    def sweep_eval(self, basis: "Basis", lasso=np.inf, want_K=False):
        """kp_sweep_eval: fit + model + validation rollout + normalised mean error of every system for one dictionary.
        Returns err (nb, n) [, K (nb, W, W)], status (nb,)."""
        err = np.zeros((self.nb, self.n)); st = np.zeros(self.nb, dtype=np.int32)
        W = basis.W
        K = np.zeros((self.nb, W, W)) if want_K else None
        las = 1e6 if (lasso is None or not np.isfinite(lasso)) else float(lasso)
        F.check(F.lib().kp_sweep_eval(self.ctx.handle, self._h, basis.handle, las, F.dptr(err), F.dptr(K), st.ctypes.data_as(F.c_ip)),
                self.ctx.handle)
        if want_K:
            return err, np.transpose(K, (0, 2, 1)), st
        return err, st

    def sweep_eval_nested(self, basis: "Basis", n_deg, lasso=np.inf):
        """kp_sweep_eval_nested: degrees 1..n_deg of the polynomial dictionary `basis` (the highest degree) from one pass
        over the data.  Returns err (n_deg, nb, n), status (n_deg, nb)."""
        err = np.zeros((n_deg, self.nb, self.n)); st = np.zeros((n_deg, self.nb), dtype=np.int32)
        las = 1e6 if (lasso is None or not np.isfinite(lasso)) else float(lasso)
        F.check(F.lib().kp_sweep_eval_nested(self.ctx.handle, self._h, basis.handle, las, int(n_deg), F.dptr(err), st.ctypes.data_as(F.c_ip)),
                self.ctx.handle)
        self._last_nested = (basis.W, int(n_deg))
        return err, st

    def nested_K(self, deg_index, W):
        """K (monomial basis, W x W per system) of degree deg_index + 1 of the most recent sweep_eval_nested call."""
        Wmax, n_deg = self._last_nested
        K = np.zeros((self.nb, W, W))
        F.check(F.lib().kp_sweep_nested_get_K(self.ctx.handle, self.nb, Wmax, n_deg, int(deg_index), int(W), F.dptr(K)), self.ctx.handle)
        return np.transpose(K, (0, 2, 1))

    def close(self):
        if self._h:
            F.lib().kp_traj_destroy(self._h)
            self._h = F.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fit_gram(ctx: Context, basis: Basis, snaps: Snapshots, fetch=True):
    W = basis.W
    if not fetch:
        F.check(F.lib().kp_fit_gram(ctx.handle, basis.handle, snaps.handle, None, None), ctx.handle)
        return None, None
    G = np.zeros((W, W), order="F"); Cm = np.zeros((W, W), order="F")
    F.check(F.lib().kp_fit_gram(ctx.handle, basis.handle, snaps.handle, F.dptr(G), F.dptr(Cm)), ctx.handle)
    return G, Cm


def fit(ctx: Context, basis: Basis, snaps: Snapshots, lasso=None, fetch=True):
    """get_Koopman on resident snapshots for each lasso value (None/inf/>=1e6 => least squares)."""
    if lasso is None:
        lasso = [np.inf]
    las = np.ascontiguousarray(np.atleast_1d(np.asarray(lasso, dtype=np.float64)))
    W = basis.W
    K = np.zeros((len(las), W, W)) if fetch else None  # each W x W block column-major
    F.check(F.lib().kp_fit(ctx.handle, basis.handle, snaps.handle, F.dptr(las), len(las), F.dptr(K)), ctx.handle)
    if not fetch:
        return None
    return [np.asfortranarray(K[i].T) for i in range(len(las))]


def fit_sharded(ctx: Context, basis: Basis, snaps_local: Snapshots, lasso=None):
    """ONE fit whose snapshot pairs are sharded over the ranks of the context's RCCL communicator (pattern 2;
    kp_fit_sharded): fused Gram kernel on the local shard, one device-to-device all-reduce of [G | C], the same solve on every
    rank - identical K everywhere.  Without a communicator this is `fit` on the local snapshots."""
    if lasso is None:
        lasso = [np.inf]
    las = np.ascontiguousarray(np.atleast_1d(np.asarray(lasso, dtype=np.float64)))
    W = basis.W
    K = np.zeros((len(las), W, W))
    F.check(F.lib().kp_fit_sharded(ctx.handle, basis.handle, snaps_local.handle, F.dptr(las), len(las), F.dptr(K)), ctx.handle)
    return [np.asfortranarray(K[i].T) for i in range(len(las))]


def fit_gram_sharded(ctx: Context, basis: Basis, snaps_local: Snapshots):
    """(G, C) of the union of the ranks' shards: local Gram kernel + one all-reduce (kp_fit_gram_sharded)."""
    W = basis.W
    G = np.zeros((W, W), order="F"); Cm = np.zeros((W, W), order="F")
    F.check(F.lib().kp_fit_gram_sharded(ctx.handle, basis.handle, snaps_local.handle, F.dptr(G), F.dptr(Cm)), ctx.handle)
    return G, Cm


def fit_refine(ctx: Context, basis: Basis, snaps: Snapshots, K, steps=1):
    """kp_fit_refine: `steps` x  K += G^-1 Px'(Py - Px K) with the residual taken from the data (QR-level accuracy for
    ill-conditioned dictionaries; MATLAB's mldivide is a QR solve, Ksysid.m:1069)."""
    Kc = F.fcol(np.array(K, dtype=np.float64))
    F.check(F.lib().kp_fit_refine(ctx.handle, basis.handle, snaps.handle, int(steps), F.dptr(Kc)), ctx.handle)
    return Kc


def _sim_marshal(ctl, ref_sc, y0_sc, u0_sc, aux_w):
    """The arguments that kp_mpc_simulate and kp_nmpc_simulate share, for the controller ctl (nproj, m): checks ref_sc and
    u0_sc against y0_sc's trial count (the caller checks the width of y0_sc itself) and allocates the outputs; aux_w is the
    width of the third output's rows (None: no such output).  Returns ((nb, nref, ref, shared, y0, u0), (U, Y, aux,
    steps_done, status), the outputs' pointers): the first and last as the library takes them (the pointers keep their
    arrays alive)."""
    y0 = np.ascontiguousarray(np.atleast_2d(y0_sc), dtype=np.float64)
    u0 = np.ascontiguousarray(np.atleast_2d(u0_sc), dtype=np.float64)
    ref = np.ascontiguousarray(ref_sc, dtype=np.float64)
    nb, n = y0.shape
    shared = ref.ndim == 2
    if ref.ndim not in (2, 3) or ref.shape[-1] != ctl.nproj or (not shared and ref.shape[0] != nb):
        raise ValueError(f"ref_sc must be (nref, {ctl.nproj}) or ({nb}, nref, {ctl.nproj}), not {ref.shape}")
    if u0.shape != (nb, ctl.m):
        raise ValueError(f"u0_sc must be ({nb}, {ctl.m}), not {u0.shape}")
    nref = ref.shape[-2]
    U = np.zeros((nb, nref, ctl.m)); Y = np.zeros((nb, nref, n))
    aux = None if aux_w is None else np.zeros((nb, max(nref - 1, 0), aux_w))
    sd = np.zeros(nb, dtype=np.int32); st = np.zeros(nb, dtype=np.int32)
    return ((nb, nref, F.dptr(ref), 1 if shared else 0, F.dptr(y0), F.dptr(u0)), (U, Y, aux, sd, st),
            (F.dptr(U), F.dptr(Y), F.dptr(aux), sd.ctypes.data_as(F.c_ip), st.ctypes.data_as(F.c_ip)))


class Mpc:
    """kp_mpc: condensed MPC problem of a linear / bilinear Koopman model on the device."""

    def __init__(self, ctx: Context, model_type, A, B, Np, proj, q_run, q_term, r, lo=None, hi=None,
                 slope_lim=None, smooth_lim=None):
        self.ctx = ctx
        ctx._children.add(self)
        A = F.fcol(A); B = F.fcol(B); proj = F.fcol(np.atleast_2d(proj))
        self.N, self.m, self.Np, self.nproj = A.shape[0], len(np.atleast_1d(r)), int(Np), proj.shape[0]
        self._zcall = None
        r = np.ascontiguousarray(np.atleast_1d(r), dtype=np.float64)
        lo_ = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
        hi_ = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
        nan = float("nan")
        self._h = F.vp()
        F.check(F.lib().kp_mpc_create(ctx.handle, F.MODEL[model_type], F.dptr(A), F.dptr(B), self.N, self.m, self.Np,
                                      F.dptr(proj), self.nproj, float(q_run), float(q_term), F.dptr(r), F.dptr(lo_),
                                      F.dptr(hi_), nan if slope_lim is None else float(slope_lim),
                                      nan if smooth_lim is None else float(smooth_lim), C.byref(self._h)), ctx.handle)
        nv, nr = C.c_int(), C.c_int()
        F.check(F.lib().kp_mpc_dims(self._h, C.byref(nv), C.byref(nr)))
        self.nvar, self.nrows = nv.value, nr.value

    @property
    def handle(self):
        return self._h

    def set_state_bounds(self, lo, hi):
        """kp_mpc_set_state_bounds: scaled-down bounds on the first n outputs (Kmpc.m:300-318); lo = None removes them."""
        if lo is None:
            F.check(F.lib().kp_mpc_set_state_bounds(self._h, 0, None, None), self.ctx.handle)
            return
        lo_ = np.ascontiguousarray(lo, dtype=np.float64); hi_ = np.ascontiguousarray(hi, dtype=np.float64)
        F.check(F.lib().kp_mpc_set_state_bounds(self._h, len(lo_), F.dptr(lo_), F.dptr(hi_)), self.ctx.handle)

    def step(self, z, u_prev, Yr, iters=1):
        """Returns (U [Np x m], status).  U is NaN when the QP failed (quadprog_gurobi.m:22-23)."""
        z = np.ascontiguousarray(z, dtype=np.float64); up = np.ascontiguousarray(u_prev, dtype=np.float64)
        yr = np.ascontiguousarray(Yr, dtype=np.float64)
        U = np.zeros((self.Np, self.m), order="F")
        st = C.c_int()
        F.check(F.lib().kp_mpc_step(self._h, F.dptr(z), F.dptr(up), F.dptr(yr), int(iters), F.dptr(U), C.byref(st)),
                self.ctx.handle)
        return U, st.value

    def step_zeta(self, basis: Basis, zeta, u_prev, Yr, iters=1):
        """One controller call with the lift fused in front (Kmpc.m:842).  This is the call inside a closed loop, so the
        marshalling is kept off its path: argument buffers and their ctypes pointers are made once per (controller,
        dictionary) and the inputs are copied into them."""
        cb = self._zcall
        if cb is None or cb[0] is not basis:
            zb = np.zeros(basis.nzeta); ub = np.zeros(self.m); yb = np.zeros(self.nproj * (self.Np + 1))
            Ub = np.zeros((self.Np, self.m), order="F"); zo = np.zeros(self.N); st = C.c_int()
            cb = self._zcall = (basis, zb, ub, yb, Ub, zo, st, F.dptr(zb), F.dptr(ub), F.dptr(yb), F.dptr(Ub), F.dptr(zo), C.byref(st),
                                F.lib().kp_mpc_step_zeta)
        _, zb, ub, yb, Ub, zo, st, pz, pu, py, pU, pzo, pst, fn = cb
        zb[...] = zeta; ub[...] = u_prev; yb[...] = Yr
        rc = fn(self._h, basis._h, pz, pu, py, int(iters), pU, pzo, pst)
        if rc:
            F.check(rc, self.ctx.handle)
        return Ub.copy(order="F"), zo.copy(), st.value

    LOAD_RATE, LOAD_PIN_LAST = 1, 2      # flags of kp_mpc_step_loaded

    def step_loaded(self, basis: Basis, nw, zeta_win, u_win, what_prev, flags, zeta, u_prev, Yr, iters=1):
        """kp_mpc_step_loaded: the load observer over the window (zeta_win: nobs + 1 rows, u_win: nobs rows; nobs = 0
        lifts with what_prev), the loaded lift of zeta and the step, one launch.  Returns (U, z, what, resnorm, status)."""
        nw = int(nw)
        zw = np.ascontiguousarray(np.atleast_2d(zeta_win) if np.size(zeta_win) else np.zeros((1, basis.nzeta)), dtype=np.float64)
        nobs = zw.shape[0] - 1
        uw = np.ascontiguousarray(np.asarray(u_win, dtype=np.float64).reshape(nobs, self.m))
        wp = None if what_prev is None else np.ascontiguousarray(np.ravel(what_prev), dtype=np.float64)
        if wp is not None and wp.size != nw:
            raise ValueError(f"what_prev must have nw = {nw} entries")
        z = np.ascontiguousarray(zeta, dtype=np.float64); up = np.ascontiguousarray(u_prev, dtype=np.float64)
        yr = np.ascontiguousarray(Yr, dtype=np.float64)
        U = np.zeros((self.Np, self.m), order="F"); zo = np.zeros(self.N); what = np.zeros(nw)
        rn = C.c_double(); st = C.c_int()
        F.check(F.lib().kp_mpc_step_loaded(self._h, basis._h, nw, nobs, F.dptr(zw), F.dptr(uw), F.dptr(wp), int(flags),
                                           F.dptr(z), F.dptr(up), F.dptr(yr), int(iters), F.dptr(U), F.dptr(zo),
                                           F.dptr(what), C.byref(rn), C.byref(st)), self.ctx.handle)
        return U, zo, what, rn.value, st.value

    def step_batch(self, Z, U_prev, YR):
        """Z (nb,N), U_prev (nb,m), YR (nb, nproj*(Np+1)) -> U (nb, Np, m), status (nb,)."""
        Z = np.ascontiguousarray(Z, dtype=np.float64); UP = np.ascontiguousarray(U_prev, dtype=np.float64)
        YR = np.ascontiguousarray(YR, dtype=np.float64)
        nb = Z.shape[0]
        U = np.zeros((nb, self.m, self.Np))          # each problem: Np x m column-major
        st = np.zeros(nb, dtype=np.int32)
        F.check(F.lib().kp_mpc_step_batch(self._h, nb, F.dptr(Z), F.dptr(UP), F.dptr(YR), F.dptr(U),
                                          st.ctypes.data_as(F.c_ip)), self.ctx.handle)
        return np.transpose(U, (0, 2, 1)), st

    def simulate(self, basis: Basis, ref_sc, y0_sc, u0_sc, iters=1, want_Z=True):
        """kp_mpc_simulate: nb closed loops with the model as the plant in one launch (Kmpc.run_simulation's loop, scaled
        units).  ref_sc: (nref, nproj) for every trial or (nb, nref, nproj); y0_sc (nb, n), u0_sc (nb, m).  Returns
        (U (nb, nref, m), Y (nb, nref, n), Z (nb, nref-1, N) or None, steps_done (nb,), status (nb,)); rows behind a failed
        step are NaN.  The kernel time is ctx.timer(F.TIMER_MPC_SIM) afterwards, ms."""
        (nb, nref, *inputs), outs, ptrs = _sim_marshal(self, ref_sc, y0_sc, u0_sc, self.N if want_Z else None)
        n = outs[1].shape[2]
        if n != basis.nzeta:       # the library reads nzeta outputs per row: a model with delays is not this loop
            raise F.KoopmanHipError(F.KP_ERR_ARG, f"kp_mpc_simulate: y0 has n = {n} entries, the dictionary's zeta has "
                                                  f"{basis.nzeta} (models with delays have no such loop)")
        F.check(F.lib().kp_mpc_simulate(self._h, basis._h, nb, nref, *inputs, int(iters), *ptrs), self.ctx.handle)
        return outs

    def last_qp(self):
        """(Hq, f, Aq, bq) of the most recent single-problem step: quadprog(Hq, f, Aq, bq)."""
        Hq = np.zeros((self.nvar, self.nvar), order="F"); f = np.zeros(self.nvar)
        Aq = np.zeros((self.nrows, self.nvar), order="F"); bq = np.zeros(self.nrows)
        F.check(F.lib().kp_mpc_last_qp(self._h, F.dptr(Hq), F.dptr(f), F.dptr(Aq), F.dptr(bq)), self.ctx.handle)
        return Hq, f, Aq, bq

    def close(self):
        if self._h:
            F.lib().kp_mpc_destroy(self._h)
            self._h = F.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Nmpc:
    """kp_nmpc: the nonlinear MPC problem of get_mpcInput_nonlinear (Kmpc.m:906-1181) on the device, one SQP per step."""

    def __init__(self, ctx: Context, basis: Basis, Kf, Np, proj, q_run, q_term, r, lo=None, hi=None, slope_lim=None,
                 smooth_lim=None):
        self.ctx = ctx
        ctx._children.add(self)
        self.basis = basis                                   # the controller evaluates this dictionary: keep it alive
        Kf = F.fcol(Kf); proj = F.fcol(np.atleast_2d(proj))
        if Kf.shape != (basis.nzeta, basis.N):
            raise ValueError(f"Kf must be nzeta x N = {basis.nzeta} x {basis.N}, it is {Kf.shape[0]} x {Kf.shape[1]}")
        if proj.shape[1] != basis.nzeta:
            raise ValueError(f"proj must have nzeta = {basis.nzeta} columns, it has {proj.shape[1]}")
        self.nzeta, self.m, self.Np, self.nproj = Kf.shape[0], basis.m, int(Np), proj.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64).ravel(), (self.m,)))
        lo_ = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
        hi_ = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
        if (lo_ is not None and lo_.size != self.m) or (hi_ is not None and hi_.size != self.m):
            raise ValueError(f"lo and hi must have m = {self.m} entries")
        nan = float("nan")
        self._h = F.vp()
        F.check(F.lib().kp_nmpc_create(ctx.handle, basis.handle, F.dptr(Kf), self.Np, F.dptr(proj), self.nproj, float(q_run),
                                       float(q_term), F.dptr(r), F.dptr(lo_), F.dptr(hi_),
                                       nan if slope_lim is None else float(slope_lim),
                                       nan if smooth_lim is None else float(smooth_lim), C.byref(self._h)), ctx.handle)
        nv, nr = C.c_int(), C.c_int()
        F.check(F.lib().kp_nmpc_dims(self._h, C.byref(nv), C.byref(nr)))
        self.nvar, self.nrows = nv.value, nr.value

    @property
    def handle(self):
        return self._h

    def set_state_bounds(self, lo, hi):
        """Scaled-down bounds on every state z_0 .. z_Np (Kmpc.m:1036-1052); lo = None removes them."""
        if lo is None:
            F.check(F.lib().kp_nmpc_set_state_bounds(self._h, 0, None, None), self.ctx.handle)
        else:
            lo_ = np.ascontiguousarray(lo, dtype=np.float64); hi_ = np.ascontiguousarray(hi, dtype=np.float64)
            if lo_.size != hi_.size:
                raise ValueError("lo and hi must have the same length")
            F.check(F.lib().kp_nmpc_set_state_bounds(self._h, len(lo_), F.dptr(lo_), F.dptr(hi_)), self.ctx.handle)
        F.check(F.lib().kp_nmpc_dims(self._h, None, C.byref(nr := C.c_int())))
        self.nrows = nr.value

    def set_options(self, max_iter=60, tol_kkt=1e-8, tol_step=1e-8, damping=10.0):
        """SQP iteration cap, stopping tolerances (KKT residual, step) and initial Levenberg-Marquardt damping."""
        F.check(F.lib().kp_nmpc_set_options(self._h, int(max_iter), float(tol_kkt), float(tol_step), float(damping)),
                self.ctx.handle)

    def step(self, zeta, u_prev, Yr, U_init=None):
        """Returns (U [Np x m], Z [(Np+1) x nzeta], info (iterations, KKT residual), status).  U is NaN when a QP
        subproblem failed; status KP_ERR_NOT_CONVERGED returns the last iterate."""
        z = np.ascontiguousarray(zeta, dtype=np.float64); up = np.ascontiguousarray(u_prev, dtype=np.float64)
        yr = np.ascontiguousarray(Yr, dtype=np.float64)
        ui = None if U_init is None else F.fcol(np.asarray(U_init, dtype=np.float64).reshape(self.Np, self.m))
        U = np.zeros((self.Np, self.m), order="F"); Z = np.zeros((self.Np + 1, self.nzeta)); info = np.zeros(2)
        st = C.c_int()
        F.check(F.lib().kp_nmpc_step(self._h, F.dptr(z), F.dptr(up), F.dptr(yr), F.dptr(ui), F.dptr(U), F.dptr(Z), F.dptr(info),
                                     C.byref(st)), self.ctx.handle)
        return U, Z, info, st.value

    def step_batch(self, zeta, u_prev, Yr, U_init=None):
        """zeta (nb, nzeta), u_prev (nb, m), Yr (nb, nproj (Np+1)), U_init (nb, Np, m) or None -> U (nb, Np, m),
        Z (nb, Np+1, nzeta), info (nb, 2), status (nb,)."""
        z = np.ascontiguousarray(zeta, dtype=np.float64); up = np.ascontiguousarray(u_prev, dtype=np.float64)
        yr = np.ascontiguousarray(Yr, dtype=np.float64)
        nb = z.shape[0]
        ui = None if U_init is None else np.ascontiguousarray(np.transpose(np.asarray(U_init, dtype=np.float64), (0, 2, 1)))
        U = np.zeros((nb, self.m, self.Np)); Z = np.zeros((nb, self.Np + 1, self.nzeta)); info = np.zeros((nb, 2))
        st = np.zeros(nb, dtype=np.int32)
        F.check(F.lib().kp_nmpc_step_batch(self._h, nb, F.dptr(z), F.dptr(up), F.dptr(yr), F.dptr(ui), F.dptr(U), F.dptr(Z),
                                           F.dptr(info), st.ctypes.data_as(F.c_ip)), self.ctx.handle)
        return np.transpose(U, (0, 2, 1)), Z, info, st

    def simulate(self, ref_sc, y0_sc, u0_sc, warm=False, want_info=True):
        """kp_nmpc_simulate: nb closed loops with the model as the plant in one launch (Kmpc.run_simulation's loop, scaled
        units).  ref_sc: (nref, nproj) for every trial or (nb, nref, nproj); y0_sc (nb, nzeta), u0_sc (nb, m).  warm: every
        step but the first starts from the previous step's solution, shifted.  Returns (U (nb, nref, m), Y (nb, nref, nzeta),
        info (nb, nref-1, 3): SQP iterations, KKT residual, status of every step (None without want_info), steps_done (nb,),
        status (nb,)); rows behind a failed step are NaN.  The kernel time is ctx.timer(F.TIMER_NMPC_SIM) afterwards, ms."""
        (nb, nref, *inputs), outs, ptrs = _sim_marshal(self, ref_sc, y0_sc, u0_sc, 3 if want_info else None)
        n = outs[1].shape[2]
        if n != self.nzeta:
            raise ValueError(f"y0_sc must be ({nb}, {self.nzeta}), not {(nb, n)}")
        F.check(F.lib().kp_nmpc_simulate(self._h, nb, nref, *inputs, 1 if warm else 0, *ptrs), self.ctx.handle)
        return outs

    def last_jacobians(self):
        """[A_k B_k] = dF/d[zeta; u] at the Np points of the last linearisation of the last single step: (Np, nzeta, nvars)."""
        nv = self.nzeta + self.m
        J = np.zeros((self.Np, nv, self.nzeta))
        F.check(F.lib().kp_nmpc_last_jacobians(self._h, F.dptr(J)), self.ctx.handle)
        return np.transpose(J, (0, 2, 1))

    def close(self):
        if self._h:
            F.lib().kp_nmpc_destroy(self._h)
            self._h = F.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
