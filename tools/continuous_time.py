"""Continuous-time models: device logm (kp_logm) and ode45 validation rollouts (kp_rollout_ct / kp_rollout_nl_ct) beside the
same work on the host (scipy.linalg.logm, the arm.dopri45 restatement).  Arm data, poly-3, dim_red (the example configuration).

    python tools/continuous_time.py [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import koopman_realizations_amd as kra  # noqa: E402
from oracle import koopman_oracle as ko  # noqa: E402
from _ct_reference import arm_trials, bilinear_rhs, linear_rhs, nonlinear_rhs, rollout_host  # noqa: E402


def best_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from scipy.linalg import logm
    ctx = kra.Context(0)
    g = {"arm_data": np.load(os.path.join(ROOT, "tests", "golden", "arm_data.npz"))}
    train, val = arm_trials(g)
    models = {}
    for mt in ("linear", "bilinear", "nonlinear"):
        ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[3], dim_red=True,
                        time_type="continuous")
        ks.train_models()
        models[mt] = ks
    Ts = models["linear"].params["Ts"]
    mats = {37: models["linear"].koopData["K"], 88: models["nonlinear"].koopData["K"], 136: models["bilinear"].koopData["K"]}
    rng = np.random.default_rng(0)
    mats[336] = np.eye(336) + 0.3 * rng.standard_normal((336, 336)) / np.sqrt(336)
    print("logm (ms, best of %d)            device    scipy   nsqrt" % a.reps)
    for n, K in mats.items():
        _, nsq, st = ctx.logm(K, 1e-12, 1.0 / Ts)
        d = best_ms(lambda: ctx.logm(K, 1e-12, 1.0 / Ts), a.reps)
        h = best_ms(lambda: logm(K + 1e-12 * np.eye(n)), a.reps)
        print(f"  n = {n:4d}{'' if n != 336 else ' (random)':9s}          {d:8.2f} {h:8.2f}   {nsq} {'' if st == 0 else 'refused'}")
    K16 = np.stack([mats[136] * (1 + 1e-4 * i) for i in range(16)])
    d = best_ms(lambda: ctx.logm(K16, 1e-12, 1.0 / Ts), a.reps)
    h = best_ms(lambda: [logm(k + 1e-12 * np.eye(136)) for k in K16], max(1, a.reps // 2))
    print(f"  16 x 136 batched               {d:8.2f} {h:8.2f}")
    print("validation (samples/s, arm val trial, RelTol 1e-3, AbsTol 1e-6)   device b=1   device b=64   host dopri45")
    for mt, ks in models.items():
        v = ks.valdata[0]
        _, yreal, ureal, zetareal = ks._val_common(v)
        T = ureal.shape[0]
        mdl = ks.model
        if mt == "nonlinear":
            one = lambda: ctx.rollout_nl_ct(ks.basis_dev, mdl["Kf"], zetareal[0], ureal, Ts)
            Kb = np.stack([mdl["Kf"]] * 64); Zb = np.stack([zetareal[0]] * 64); Ub = np.stack([ureal] * 64)
            many = lambda: ctx.rollout_nl_ct(ks.basis_dev, Kb, Zb, Ub, Ts)
            dic = ko.Dictionary("nonlinear", 6, 3, ko.make_basis(9, ["poly"], [3]), ks.basis["pcs"])
            rhs, x0 = nonlinear_rhs(dic, mdl["Kf"]), zetareal[0]
        else:
            z0 = ks.lift.econ_full(zetareal[0])
            one = lambda: ctx.rollout_ct(mt, mdl["A"], mdl["B"], z0, ureal, 6, Ts)
            Ab = np.stack([mdl["A"]] * 64); Bb = np.stack([mdl["B"]] * 64); Zb = np.stack([z0] * 64); Ub = np.stack([ureal] * 64)
            many = lambda: ctx.rollout_ct(mt, Ab, Bb, Zb, Ub, 6, Ts)
            rhs, x0 = (linear_rhs if mt == "linear" else bilinear_rhs)(mdl["A"], mdl["B"]), z0
        d1 = best_ms(one, a.reps); d64 = best_ms(many, a.reps)
        Th = 41
        hh = best_ms(lambda: rollout_host(rhs, x0, ureal[:Th], Ts), 1)
        print(f"  {mt:9s} ({T - 1} intervals)          {1e3 * (T - 1) / d1:10.0f} {64e3 * (T - 1) / d64:13.0f} {1e3 * (Th - 1) / hh:14.0f}")
    ctx.close()


if __name__ == "__main__":
    main()
