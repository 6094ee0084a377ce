"""Lasso fits in a fresh interpreter: the solver's environment switches (KP_LASSO_NO_POLISH, KP_LASSO_PATH_AFTER,
KP_LASSO_NO_FUSED, KP_LASSO_ROUNDS, ...) are read once per process, so a test that needs one of them starts a child with it set.

in_fresh_process(problems, env): problems = [(G, C, T), ...] with T a (calls, values) array of L1 budgets - every row of T is
one kp_fit_lasso_batch call on (G, C).  Returns per problem a dict K (calls, values, W, ncols), it (calls, values), ms (calls:
kp_timer_get(11) behind the call) and mask (calls: kp_timer_get(27)).  tol: the convergence tolerance of every call.  The child is this file run as a script."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def in_fresh_process(problems, env, timeout=600, tol=1e-10):
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        arrays = {"n": np.array(len(problems)), "tol": np.array(float(tol))}
        for i, (G, C, T) in enumerate(problems):
            arrays.update({f"G{i}": G, f"C{i}": C, f"T{i}": np.atleast_2d(np.asarray(T, dtype=float))})
        np.savez(src, **arrays)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), ROOT, src, dst], env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=timeout)
        assert r.returncode == 0, r.stderr[-2000:]
        o = np.load(dst)
        return [{k: o[f"{k}{i}"] for k in ("K", "it", "ms", "mask")} for i in range(len(problems))]


def _child(root, src, dst):
    sys.path.insert(0, root)
    import koopman_realizations_amd as kra
    d = np.load(src)
    c = kra.Context(0)
    out = {}
    for i in range(int(d["n"])):
        G, C, T = d[f"G{i}"], d[f"C{i}"], d[f"T{i}"]
        Ks, its, ms, mask = [], [], [], []
        for t in T:
            K, it = c.fit_lasso_batch(G, C, t, tol=float(d["tol"]))
            Ks.append(np.stack(K)); its.append(it); ms.append(c.timer(11)); mask.append(c.timer(27))
        out.update({f"K{i}": np.stack(Ks), f"it{i}": np.stack(its), f"ms{i}": np.array(ms), f"mask{i}": np.array(mask)})
    np.savez(dst, **out)
    c.close()


if __name__ == "__main__":
    _child(*sys.argv[1:4])
