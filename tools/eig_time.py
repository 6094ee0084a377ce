"""The batched device eigensolver (kp_eig, Context.eig) beside numpy.linalg.eig / eigvals on the same machine.  Gaussian
matrices:

  * single matrices n = 33, 88, 136, 336
  * batches 16 x 33, 16 x 136 (a lasso grid's candidates) and 1 024 x 10 (the random-system sweep's shape)

each with values only and with vectors.  Best of --reps runs: a host clock around the whole call (upload, kernel, results
back, the sort), the kernel's own time (kp_timer_get(22)) and the regime it ran (kp_timer_get(23)); the host's LAPACK over
the same stack.  One matrix alone is a serial bulge chase and latency-bound: these are records, not thresholds.

    python tools/eig_time.py [--reps 5] [--out profiles/eig_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import koopman_realizations_amd as kra  # noqa: E402
from koopman_realizations_amd import _ffi as F  # noqa: E402

SHAPES = [(1, 33), (1, 88), (1, 136), (1, 336), (16, 33), (16, 136), (1024, 10)]


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_time.json"))
    a = ap.parse_args()
    ctx = kra.Context(0)
    rng = np.random.default_rng(0)
    rows = []
    for nb, n in SHAPES:
        A = rng.standard_normal((nb, n, n))
        for vectors in (False, True):
            lam, V, it, st = ctx.eig(A, vectors=vectors)          # warm-up: the workspace and the kernel are there
            assert np.all(st == F.KP_OK)
            tk = []

            def dev():
                ctx.eig(A, vectors=vectors)
                tk.append(ctx.timer(F.TIMER_EIG))
            wall = best(dev, a.reps)
            host = best((lambda: np.linalg.eig(A)) if vectors else (lambda: np.linalg.eigvals(A)), a.reps)
            ref = np.linalg.eigvals(A[0])
            d = np.abs(lam[0][:, None] - ref[None, :]).min(axis=1).max()
            rows.append({"nb": nb, "n": n, "vectors": vectors, "regime": int(ctx.timer(F.TIMER_EIG_REGIME)), "device_wall_ms": wall * 1e3,
                         "device_kernel_ms": min(tk), "numpy_ms": host * 1e3, "qr_iterations_mean": float(np.mean(it)),
                         "max_eigenvalue_distance_to_lapack_matrix_0": float(d)})
    out = {"workload": "kp_eig on Gaussian matrices beside numpy.linalg.eig / eigvals (LAPACK, host threads as configured)",
           "device": ctx.info(), "reps": a.reps, "rows": rows}
    print("%6s %5s %8s %7s %16s %16s %12s" % ("nb", "n", "vectors", "regime", "device wall ms", "device kernel ms", "numpy ms"))
    for r in rows:
        print("%6d %5d %8s %7d %16.3f %16.3f %12.3f" % (r["nb"], r["n"], "yes" if r["vectors"] else "no", r["regime"], r["device_wall_ms"],
                                                       r["device_kernel_ms"], r["numpy_ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, default=str)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
