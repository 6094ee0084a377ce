#!/usr/bin/env python3
"""Per-step cost of a loaded controller step: the fused kp_mpc_step_loaded (load observer + loaded lift + MPC step in
one launch) against the host-assembled path (estimate_load_bilinear: lift of the window, numpy regression, kp_qp_solve;
then the loaded lift and kp_mpc_step), with the unloaded kp_mpc_step_zeta of a model of the same dictionary for scale.

Wall time per step on the host (median over --steps calls after --warmup) and the kernel time of the step launch
(Context.timer(2): the step kernel's device time).  Model: the toy loaded system of tests/_loaded_system.py, bilinear
poly-3, nw = 1, horizon 10, a window of load_obs_horizon + 1 = 11 samples.

    python tools/loaded_step_time.py [--steps 400] [--warmup 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import koopman_realizations_amd as kra  # noqa: E402
from tests._loaded_system import make_trials  # noqa: E402


def controller(loaded):
    trials = make_trials(14, 200, nw=1, seed=21)
    if not loaded:
        trials = [{k: v for k, v in t.items() if k != "w"} for t in trials]
    ks = kra.Ksysid({"train": trials[:12], "val": trials[12:]}, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    loaded=loaded)
    ks.train_models()
    return kra.Kmpc(ks, horizon=10, input_bounds=[-2.0, 2.0], cost_running=10.0, cost_terminal=100.0, cost_input=0.01,
                    projmtx=ks.model["C"][:2])


def timed(fn, steps, warmup, ctx):
    wall, kern = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        fn(i)
        t1 = time.perf_counter()
        if i >= warmup:
            wall.append((t1 - t0) * 1e6)
            kern.append(ctx.timer(2) * 1e3)
    return float(np.median(wall)), float(np.median(kern))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    mpc, mpc0 = controller(True), controller(False)
    ks = mpc.sysid
    ctx = ks.ctx
    v = ks.valdata[0]
    ref = np.column_stack([0.4 * np.sin(np.arange(11) * 0.1), 0.4 * np.cos(np.arange(11) * 0.1)])
    H = mpc.load_obs_horizon + 1

    def window(i):
        t = H + i % (v["y"].shape[0] - H - 1)
        return {"y": v["y"][t:t + 1], "u": v["u"][t:t + 1]}, v["y"][t + 1 - H:t + 1], v["u"][t + 1 - H:t + 1]

    def fused(i):
        traj, yp, up = window(i)
        mpc.get_mpcInput_loaded(traj, ref, yp, up)

    def host(i):
        traj, yp, up = window(i)
        traj["what"] = mpc.estimate_load_bilinear(yp, up)[0][None, :]
        mpc._step(traj, ref, 1)

    def unloaded(i):
        traj, _, _ = window(i)
        mpc0.get_mpcInput_bilinear_iter(traj, ref, 1)

    out = {"N": ks.params["N"], "nw": ks.params["nw"], "window": H, "horizon": mpc.horizon}
    for name, fn in (("fused_loaded", fused), ("host_loaded", host), ("unloaded_step_zeta", unloaded)):
        w, k = timed(fn, a.steps, a.warmup, ctx)
        out[name] = {"wall_us": round(w, 1), "step_kernel_us": round(k, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
