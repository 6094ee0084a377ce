"""Whole closed loops in one launch (kp_mpc_simulate, Kmpc.run_simulations) beside the host loop Kmpc.run_simulation.
The arm's bilinear controller (example_control.m settings, N = 34, horizon 10) on the block-M reference, 300 steps, the
identified model as the plant:

  * the host loop run_simulation: one launch per step
  * one launch at nb = 1, 64, 1 024 and 4 096 trials (the starts of the batch are perturbed copies of the first)

Best of --reps runs each: host wall time of the whole call and the kernel's own time (kp_timer_get(19)); trials x steps per
second from both.  Z is not asked for beyond one trial (4 096 trials of it are 333 MB of output).

    python tools/mpc_sim_time.py [--reps 5] [--out profiles/mpc_sim_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_sim_time.json"))
    a = ap.parse_args()
    ctx = kra.Context(0)
    gd = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(gd, "arm_data.npz")); ref = np.load(os.path.join(gd, "blockM_ref.npz"))["y"]
    y0 = np.load(os.path.join(gd, "arm_blockM.npz"))["bilin_Y"][0]
    off = np.concatenate([[0], np.cumsum(g["train_len"])])
    train = [{"t": g["train_t"][i:j], "y": g["train_y"][i:j], "u": g["train_u"][i:j]} for i, j in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()
    mpc = kra.Kmpc(ks, horizon=10, input_bounds=[-7 * np.pi / 8, 7 * np.pi / 8], input_slopeConst=1e-1, input_smoothConst=None,
                   state_bounds=None, cost_running=10, cost_terminal=100, cost_input=0.1 * np.array([3e-2, 2e-2, 1e-2]),
                   projmtx=ks.model["C"][-2:, :])
    nref = ref.shape[0]
    steps = nref - 1
    rows = []
    # the host loop
    mpc.run_simulation(ref[:20], y0)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); host = mpc.run_simulation(ref, y0); ts.append(time.perf_counter() - t0)
    assert len(host["comp_time"]) == steps
    rows.append({"route": "run_simulation (host loop, one launch per step)", "nb": 1, "wall_ms": min(ts) * 1e3, "kernel_ms": None,
                 "trial_steps_per_s_wall": steps / min(ts), "trial_steps_per_s_kernel": None})
    # one launch
    ref_sc = mpc.scaledown_ref(ref)
    y0_sc, u0_sc = ks.scaledown_y(y0), ks.scaledown_u(np.zeros(3))
    rng = np.random.default_rng(0)
    dev1 = None
    for nb in (1, 64, 1024, 4096):
        Y0 = y0_sc + np.concatenate([np.zeros((1, 6)), 0.02 * rng.standard_normal((nb - 1, 6))])
        U0 = np.tile(u0_sc, (nb, 1))
        want_Z = nb == 1
        mpc.dev.simulate(ks.basis_dev, ref_sc, Y0, U0, 1, want_Z)
        tw, tk = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            U, Y, Z, sd, st = mpc.dev.simulate(ks.basis_dev, ref_sc, Y0, U0, 1, want_Z)
            tw.append(time.perf_counter() - t0); tk.append(ctx.timer(F.TIMER_MPC_SIM) * 1e-3)
        done = int(sd.sum())
        rows.append({"route": "kp_mpc_simulate (one launch)", "nb": nb, "wall_ms": min(tw) * 1e3, "kernel_ms": min(tk) * 1e3,
                     "trial_steps_per_s_wall": done / min(tw), "trial_steps_per_s_kernel": done / min(tk),
                     "trials_completed": int((sd == steps).sum()), "us_per_step_kernel_one_trial": min(tk) * 1e6 / steps if nb == 1 else None})
        if nb == 1:
            dev1 = (U, Y)
    dY = float(np.abs(ks.scaleup_y(dev1[1][0]) - host["Y"]).max())
    out = {"workload": "bilinear Kmpc, horizon 10, block-M reference, %d steps, arm model N = %d (poly-3, dim_red), model as plant" %
                       (steps, int(ks.params["N"])),
           "device": ctx.info(), "reps": a.reps, "one_launch_vs_host_loop_max_abs_dY": dY, "rows": rows}
    print("%-52s %6s %12s %12s %16s %16s" % ("route", "nb", "wall ms", "kernel ms", "trial-steps/s wall", "kernel"))
    for r in rows:
        print("%-52s %6d %12.3f %12s %16.0f %16s" % (r["route"], r["nb"], r["wall_ms"], "-" if r["kernel_ms"] is None else "%.3f" % r["kernel_ms"],
                                                     r["trial_steps_per_s_wall"],
                                                     "-" if r["trial_steps_per_s_kernel"] is None else "%.0f" % r["trial_steps_per_s_kernel"]))
    print("one launch vs host loop, max |dY| over the run (output units): %.3e" % dY)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, default=str)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
