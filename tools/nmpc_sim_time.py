"""Whole nonlinear-MPC closed loops in one launch (kp_nmpc_simulate, Kmpc.run_simulations) beside the routes that existed
before it.  The arm's nonlinear controller (example_control.m settings: poly-3, dim_red, N = 88, horizon 10, slope constant
1e-1, input_bounds = []) on the block-M reference, 300 steps, the identified model as the plant:

  * the host loop Kmpc.run_simulation, 1 trial: one kp_nmpc_step launch per step, the plant step on the host;
  * one launch at nb = 1, 64, 256 and 1 024 trials, cold (every step from the reference's start X0) and warm (from the
    previous step's solution, shifted);
  * for the same batches the lockstep route: a Python loop of Nmpc.step_batch calls, one per step - every trial waits at
    every step for the slowest SQP of the batch.

Trial i of a batch follows the reference shifted by i mod 16 rows (its last row repeated behind the end) from the stored
run's state at that row, perturbed: distinct starts, distinct references.  Best of --reps runs each: host wall time of the
whole call and, for the one-launch route, the kernel's own time (kp_timer_get(21)).

    python tools/nmpc_sim_time.py [--reps 5] [--steps 300] [--out profiles/nmpc_sim_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import koopman_realizations_amd as kra  # noqa: E402
from koopman_realizations_amd import _ffi as F  # noqa: E402
from nmpc_step_time import GOLDEN, arm_sysid, controller, status_counts  # noqa: E402


def lockstep(dev, ref, Y0, U0, warm):
    """The closed loops of a batch through kp_nmpc_step_batch, one launch per step."""
    nb, nref, Np = Y0.shape[0], ref.shape[1], dev.Np
    zeta, up, Uprev = Y0, U0, None
    Y, U, sts = [Y0], [U0], []
    for k in range(1, nref):
        idx = np.minimum(np.arange(k - 1, k + Np), nref - 1)
        init = None if (not warm or Uprev is None) else np.concatenate([Uprev[:, 1:], Uprev[:, -1:]], axis=1)
        Uprev, Z, info, st = dev.step_batch(zeta, up, ref[:, idx].reshape(nb, -1), init)
        zeta, up = Z[:, 1], Uprev[:, 1]
        Y.append(zeta); U.append(up); sts.append(st)
    return np.stack(U, axis=1), np.stack(Y, axis=1), np.array(sts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--batches", default="1,64,256,1024")
    ap.add_argument("--step-ab", default=None, help="JSON file with the single step's parent / change timings, copied into the output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmpc_sim_time.json"))
    a = ap.parse_args()
    ctx = kra.Context(0)
    ks = arm_sysid(ctx)
    mpc = {False: controller(ks, a, False), True: controller(ks, a, True)}
    d = np.load(os.path.join(GOLDEN, "arm_nmpc.npz"))
    ref = np.load(os.path.join(GOLDEN, "blockM_ref.npz"))["y"][:a.steps + 1]
    nref, steps = ref.shape[0], ref.shape[0] - 1
    rows = []

    def say(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    # the host loop
    y0 = d["Y"][0]
    mpc[False].run_simulation(ref[:10], y0, np.zeros(3))
    host = {}
    for warm in (False, True):
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); host[warm] = mpc[warm].run_simulation(ref, y0, np.zeros(3)); ts.append(time.perf_counter() - t0)
        done = len(host[warm]["comp_time"])
        say({"route": "run_simulation (host loop, one launch per step)", "start": "warm" if warm else "cold", "nb": 1,
             "wall_ms": min(ts) * 1e3, "kernel_ms": None, "trial_steps_per_s_wall": done / min(ts), "steps_done": done,
             "step_statuses": status_counts(host[warm]["nmpc_info"][:, 2])})
    ref_sc = mpc[False].scaledown_ref(ref)
    rng = np.random.default_rng(0)
    dev = mpc[False].dev
    one = {}
    for nb in [int(x) for x in a.batches.split(",")]:
        shift = np.arange(nb) % 16
        R = np.stack([ref_sc[np.minimum(np.arange(nref) + s, nref - 1)] for s in shift])
        pert = np.concatenate([np.zeros((1, 9)), 0.005 * rng.standard_normal((nb - 1, 9))])
        Y0 = ks.scaledown_y(d["Y"][shift]) + pert[:, :6]
        U0 = ks.scaledown_u(d["U"][shift]) + pert[:, 6:]
        for warm in (False, True):
            dev.simulate(R, Y0, U0, warm=warm)
            tw, tk = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                U, Y, info, sd, st = dev.simulate(R, Y0, U0, warm=warm)
                tw.append(time.perf_counter() - t0); tk.append(ctx.timer(F.TIMER_NMPC_SIM) * 1e-3)
            done = int(sd.sum())
            its = info[:, :, 0][np.isfinite(info[:, :, 0])]
            say({"route": "kp_nmpc_simulate (one launch)", "start": "warm" if warm else "cold", "nb": nb, "wall_ms": min(tw) * 1e3,
                 "kernel_ms": min(tk) * 1e3, "trial_steps_per_s_wall": done / min(tw), "trial_steps_per_s_kernel": done / min(tk),
                 "trials_completed": int((sd == steps).sum()), "trial_statuses": status_counts(st),
                 "sqp_iterations_mean": float(its.mean()), "sqp_iterations_max": int(its.max()),
                 "ms_per_step_kernel_one_trial": min(tk) * 1e3 / steps if nb == 1 else None})
            if nb == 1:
                one[warm] = (U, Y)
            lockstep(dev, R[:, :5], Y0, U0, warm)
            tl = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); Ul, Yl, stl = lockstep(dev, R, Y0, U0, warm); tl.append(time.perf_counter() - t0)
            ok = np.isfinite(Ul).all(axis=(1, 2))
            both = ok & (sd == steps)
            say({"route": "Python loop of step_batch (lockstep, one launch per step)", "start": "warm" if warm else "cold", "nb": nb,
                 "wall_ms": min(tl) * 1e3, "kernel_ms": None, "trial_steps_per_s_wall": int(ok.sum()) * steps / min(tl),
                 "trials_completed": int(ok.sum()), "step_statuses": status_counts(stl),
                 "max_abs_dU_vs_one_launch_completed_trials": float(np.abs(Ul[both] - U[both]).max()) if both.any() else None})
    sy, su = ks.scaledown_y, ks.scaledown_u
    diffs = {("warm" if w else "cold"): float(max(np.abs(one[w][1][0] - sy(host[w]["Y"])).max(), np.abs(one[w][0][0] - su(host[w]["U"])).max()))
             for w in one if len(host[w]["K"]) == nref}
    out = {"workload": "nonlinear Kmpc, horizon 10, slope 1e-1, block-M reference, %d steps, arm model N = %d (poly-3, dim_red), model as "
                       "plant; nmpc_max_iter %d, nmpc_tol %g" % (steps, int(ks.params["N"]), a.max_iter, a.tol),
           "device": ctx.info(), "reps": a.reps, "one_launch_vs_host_loop_max_abs_diff_scaled": diffs, "rows": rows}
    if a.step_ab:
        with open(a.step_ab) as f:
            out["single_step_parent_vs_change"] = json.load(f)
    print("%-58s %5s %6s %12s %12s %18s" % ("route", "start", "nb", "wall ms", "kernel ms", "trial-steps/s wall"))
    for r in rows:
        print("%-58s %5s %6d %12.1f %12s %18.0f" % (r["route"], r["start"], r["nb"], r["wall_ms"],
                                                   "-" if r["kernel_ms"] is None else "%.1f" % r["kernel_ms"], r["trial_steps_per_s_wall"]))
    print("one launch vs host loop, one trial, max difference in scaled units:", diffs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, default=str)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
