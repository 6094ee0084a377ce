"""The arm plant on the device (kp_arm_simulate, kra.DeviceArm) beside the host plant (arm.py).  The stored arm
(3 links, 60 s trials at 20 Hz = 1 201 samples, stored training inputs cycled over the batch):

  * SPAN_ZOH trials/s and samples/s at batch 1, 10, 64, 1 024 and 16 384 (one launch per batch)
  * the host yardstick arm.ode45_span on one trial (--host-samples of it; the full trial takes ~45 s)
  * one closed-loop Ksim trial (example_control.m, bilinear, block-M reference) with the host Arm and with DeviceArm

    python tools/arm_sim_time.py [--reps 3] [--host-samples 200]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import koopman_realizations_amd as kra  # noqa: E402
from _arm_span_reference import host_span  # noqa: E402


def best_s(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-samples", type=int, default=200)
    a = ap.parse_args()
    ctx = kra.Context(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "arm_data.npz"))
    gp = np.load(os.path.join(ROOT, "tests", "golden", "arm_plant.npz"))
    params = {k[2:]: (float(gp[k]) if gp[k].ndim == 0 else gp[k]) for k in gp.files if k.startswith("p_")}
    arm = kra.Arm(params, "markers")
    darm = kra.DeviceArm(params, "markers", ctx=ctx)
    t = g["train_t"][:1201, 0]
    off = np.concatenate([[0], np.cumsum(g["train_len"])])
    U10 = np.stack([g["train_u"][a_:b_] for a_, b_ in zip(off[:-1], off[1:])])
    print("SPAN_ZOH, 60 s trials (1 201 samples)    batch   seconds   trials/s    samples/s   mean accepted steps")
    for b in (1, 10, 64, 1024, 16384):
        U = U10[np.arange(b) % 10]
        s = best_s(lambda: ctx.arm_simulate(params, "zoh", t, U), a.reps if b < 16384 else 1)
        _, na, _, st = ctx.arm_simulate(params, "zoh", t, U)
        assert (st == 0).all()
        print(f"{'':40s}{b:6d} {s:9.3f} {b / s:10.1f} {b * 1201 / s:12.0f}   {na.mean():.0f}")
    n = a.host_samples
    t0 = time.perf_counter()
    host_span(arm, t[:n], U10[0, :n])
    hs = time.perf_counter() - t0
    print(f"host ode45_span, one trial, {n} samples: {hs:.2f} s ({n / hs:.1f} samples/s; a 1 201-sample trial ~{hs * 1201 / n:.0f} s)")

    from test_gpu_arm_plant import _example_control
    golden = {"arm_data": g, "arm_plant": gp}
    ref = np.load(os.path.join(ROOT, "tests", "golden", "blockM_ref.npz"))["y"]
    for cls in (kra.Arm, kra.DeviceArm):
        _, sim = _example_control(ctx, golden, cls)
        t0 = time.perf_counter()
        res = sim.run_trial_mpc(ref, None, None)
        el = time.perf_counter() - t0
        print(f"closed loop, block-M (300 steps), plant {cls.__name__:9s}: {el:6.2f} s  ({1e3 * el / 300:.2f} ms per step, "
              f"mean MPC step {1e3 * np.mean(res['comp_time']):.3f} ms)")
    one = best_s(lambda: darm.simulate_Ts(gp["bilin_X"][5], gp["bilin_U"][5]), 20)
    print(f"DeviceArm.simulate_Ts, one call: {1e3 * one:.3f} ms")


if __name__ == "__main__":
    main()
