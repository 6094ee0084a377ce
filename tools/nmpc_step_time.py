#!/usr/bin/env python3
"""Cost of the nonlinear MPC step (kp_nmpc_step) on example_control.m's nonlinear arm controller (poly-3, dim_red, N = 88,
horizon 10, slope constant 1e-1, input_bounds = [] as in the stored run res_nonlin).

  * teacher-forced over the 299 stored states of res_nonlin (tests/golden/arm_nmpc.npz): wall time per step (median),
    SQP iterations per step (median / max / steps at the cap) and the statuses - cold (the reference's start X0) and
    warm-started (the previous step's solution shifted by one step);
  * the free-running closed loop on the arm plant (Ksim.run_trial_mpc): comp_time, mean tracking error, statuses;
  * batch throughput: kp_nmpc_step_batch over --batch problems (the stored states, repeated).

Prints one JSON object.  Run under `rocprofv3 --kernel-trace --stats` for the kernel time of kp_nmpc_kernel.

    python tools/nmpc_step_time.py [--batch 1024] [--max-iter 60] [--tol 1e-8]
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
from koopman_realizations_amd import _ffi as F  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def arm_sysid(ctx):
    g = np.load(os.path.join(GOLDEN, "arm_data.npz"))
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    return kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="nonlinear", obs_type=["poly"], obs_degree=[3],
                      snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()


def controller(ks, args, warm=False, **kw):
    opts = dict(horizon=10, input_bounds=[], input_slopeConst=1e-1, cost_running=10, cost_terminal=100,
                cost_input=0.1 * np.array([3e-2, 2e-2, 1e-2]), projmtx=ks.model["C"][-2:, :], mpc_type="nonlinear",
                nmpc_max_iter=args.max_iter, nmpc_tol=args.tol, nmpc_warm_start=warm)
    opts.update(kw)
    return kra.Kmpc(ks, **opts)


def status_counts(st):
    names = {F.KP_OK: "ok", F.KP_ERR_NOT_CONVERGED: "not_converged", F.KP_ERR_QP_FAIL: "qp_fail"}
    v, c = np.unique(np.asarray(st), return_counts=True)
    return {names.get(int(a), str(int(a))): int(b) for a, b in zip(v, c)}


def replay(ks, args, warm):
    d = np.load(os.path.join(GOLDEN, "arm_nmpc.npz"))
    ref = np.load(os.path.join(GOLDEN, "blockM_ref.npz"))["y"]
    mpc = controller(ks, args, warm)
    ref_sc = mpc.scaledown_ref(ref)
    wall, its, st, dev = [], [], [], []
    for k in range(299):
        cur = {"y": ks.scaledown_y(d["Y"][k])[None, :], "u": ks.scaledown_u(d["U"][k])[None, :]}
        t0 = time.perf_counter()
        U, _ = mpc.get_mpcInput_nonlinear(cur, ref_sc[k:k + 11])
        wall.append(time.perf_counter() - t0)
        its.append(mpc.last_info[0]); st.append(mpc.last_info[2])
        dev.append(float(np.abs(ks.scaleup_u(U[1]) - d["U"][k + 1]).max()))
    its = np.array(its)
    return {"us_per_step_median": 1e6 * float(np.median(wall)), "us_per_step_mean": 1e6 * float(np.mean(wall)),
            "iterations_median": float(np.median(its)), "iterations_p90": float(np.percentile(its, 90)),
            "iterations_max": int(its.max()), "steps_at_cap": int((its >= args.max_iter).sum()), "statuses": status_counts(st),
            "U2_vs_stored_median": float(np.median(dev)), "U2_vs_stored_max": float(np.max(dev)),
            "iterations": its.tolist()}


def loop(ks, args, box):
    from koopman_realizations_amd.arm import Arm
    g = np.load(os.path.join(GOLDEN, "arm_plant.npz"))
    params = {k[2:]: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files if k.startswith("p_")}
    ref = np.load(os.path.join(GOLDEN, "blockM_ref.npz"))["y"]
    d = np.load(os.path.join(GOLDEN, "arm_nmpc.npz"))
    kw = {"input_bounds": [-7 * np.pi / 8, 7 * np.pi / 8]} if box else {}
    res = kra.Ksim(Arm(params, output_type="markers"), controller(ks, args, **kw)).run_trial_mpc(ref)
    info = np.array([i[0] for i in res["nmpc_info"]])
    out = {"steps": int(len(res["err"])), "mean_err": float(np.mean(res["err"])),
           "comp_time_ms_median": 1e3 * float(np.median(res["comp_time"])), "comp_time_ms_mean": 1e3 * float(np.mean(res["comp_time"])),
           "iterations_median": float(np.median(info)), "iterations_max": int(info.max()),
           "statuses": status_counts([i[2] for i in res["nmpc_info"]])}
    if not box:
        dev = np.abs(res["U"] - d["U"]).max(axis=1)
        out["steps_on_stored_U_1e-6"] = int(np.argmax(dev > 1e-6)) if (dev > 1e-6).any() else len(dev)
        out["steps_on_stored_U_1e-3"] = int(np.argmax(dev > 1e-3)) if (dev > 1e-3).any() else len(dev)
        out["max_dev_Y"] = float(np.abs(res["Y"] - d["Y"]).max())
    return out


def batch(ks, args):
    d = np.load(os.path.join(GOLDEN, "arm_nmpc.npz"))
    ref = np.load(os.path.join(GOLDEN, "blockM_ref.npz"))["y"]
    mpc = controller(ks, args)
    ref_sc = mpc.scaledown_ref(ref)
    idx = np.arange(args.batch) % 290                                        # (states with a full reference horizon)
    Z0 = ks.scaledown_y(d["Y"][idx]); UP = ks.scaledown_u(d["U"][idx])
    YR = np.array([ref_sc[k:k + 11].ravel() for k in idx])
    mpc.dev.step_batch(Z0, UP, YR)                                           # warm-up (first launch, pinned buffers)
    t0 = time.perf_counter()
    _, _, info, st = mpc.dev.step_batch(Z0, UP, YR)
    dt = time.perf_counter() - t0
    return {"problems": args.batch, "seconds": dt, "problems_per_s": args.batch / dt, "iterations_max": int(info[:, 0].max()),
            "statuses": status_counts(st)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--tol", type=float, default=1e-8)
    args = ap.parse_args()
    ctx = kra.Context(0)
    ks = arm_sysid(ctx)
    out = {"cold": replay(ks, args, False), "warm": replay(ks, args, True), "loop": loop(ks, args, False),
           "loop_box_7pi8": loop(ks, args, True), "batch": batch(ks, args), "max_iter": args.max_iter, "tol": args.tol}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
