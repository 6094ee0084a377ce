"""The random-system generator on the device (kp_rsys_simulate, kra.DeviceRsys) beside the host mirror, at the bench's
shape: 1 024 systems (3 terms, degree_x 3, degree_u 2) x 11 trials x 1 001 samples (Ts = 0.01), in both modes:

  * device generation: the trajectories back to the host (kernel time and wall time), and straight into a Traj
  * Rsys.simulate_systems_fast on the host (restart mode only: the host has no span form at this size)
  * generation + sweep.rand_models_sweep_traj (all 23 fits + validations of evaluate_rand_models.m) end to end

Every step runs in a child process of its own under `timeout -k 10`; the first step that fails or times out ends the
run.  The table goes to stdout and, with --out, the figures as JSON to that file.

    python tools/rsys_gen_time.py [--reps 3] [--systems 1024] [--out FILE.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
SHAPE = (3, 3, 2)
LIMITS = {"device": 300, "host": 900, "e2e": 600}


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return min(ts)


def step(name, mode, nsys, reps):
    sys.path.insert(0, ROOT)
    import koopman_realizations_amd as kra
    from koopman_realizations_amd import sweep
    from koopman_realizations_amd.rsys import Rsys
    x0 = np.zeros((1, 1))
    out = {"step": name, "mode": mode, "systems": nsys}
    if name == "host":
        r = Rsys(nsys, *SHAPE, seed=1)
        t0 = time.perf_counter()
        r.simulate_systems_fast(10.0, 0.01, 11, x0)
        out["host_s"] = time.perf_counter() - t0
        return out
    ctx = kra.Context(0)
    try:
        d = kra.DeviceRsys(nsys, *SHAPE, seed=1, ctx=ctx)
        if name == "device":
            fn = d.simulate_systems if mode == "span" else d.simulate_systems_restart
            out["to_host_s"] = best(lambda: fn(10.0, 0.01, 11, x0), reps)
            out["kernel_ms"] = ctx.timer(5)
            steps = d.last_stats["naccept"] + d.last_stats["nreject"]
            out["steps_mean"], out["steps_max"] = float(steps.mean()), int(steps.max())

            def to_traj():
                d.simulate_to_traj(10.0, 0.01, 11, x0, mode=mode).close()
            out["to_traj_s"] = best(to_traj, reps)
        else:
            def e2e():
                traj = d.simulate_to_traj(10.0, 0.01, 11, x0, mode=mode)
                try:
                    tab = sweep.rand_models_sweep_traj(traj, ctx)
                finally:
                    traj.close()
                return tab
            out["e2e_s"] = best(e2e, reps)
    finally:
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--systems", type=int, default=1024)
    ap.add_argument("--out", default=None, help="write the figures as JSON to this file")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="span", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.mode, a.systems, a.reps)), flush=True)
        return
    plan = [("device", "span"), ("device", "restart"), ("e2e", "span"), ("e2e", "restart"), ("host", "restart")]
    res = []
    for name, mode in plan:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--mode", mode,
               "--systems", str(a.systems), "--reps", str(a.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(f"step {name}/{mode} failed with exit status {p.returncode}; stopping.\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            break
        res.append(json.loads(lines[-1][7:]))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    n = a.systems
    print(f"\n{n} systems x 11 trials x 1 001 samples")
    print("| mode | kernel | generation, Y to host | generation into a Traj | + sweep (23 fits + validations) | host simulate_systems_fast | mean / max steps per trial |")
    print("|---|---|---|---|---|---|---|")
    by = {(r["step"], r["mode"]): r for r in res}
    for mode in ("span", "restart"):
        dv, e2, ho = by.get(("device", mode), {}), by.get(("e2e", mode), {}), by.get(("host", mode), {})
        f = lambda v, s=1e3, u="ms": f"{v * s:.1f} {u}" if v is not None else "-"
        print(f"| {mode} | {f(dv.get('kernel_ms'), 1)} | {f(dv.get('to_host_s'))} | {f(dv.get('to_traj_s'))} | {f(e2.get('e2e_s'))} | "
              f"{f(ho.get('host_s'), 1, 's')} | {dv.get('steps_mean', 0):.0f} / {dv.get('steps_max', 0)} |")
    if len(res) != len(plan):
        sys.exit(1)


if __name__ == "__main__":
    main()
