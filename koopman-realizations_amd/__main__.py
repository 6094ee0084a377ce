"""Command line: identify a Koopman model from a reference data file, without MATLAB.

    python -m koopman_realizations_amd sysid DATA.mat --model_type bilinear --obs_degree 3 [--dim_red]
        [--time_type continuous] [--lasso 1 10 100 --metric euclid_mean [--horizon 10 [--horizon_stride 1]]] [--spectrum]
        [--out model.npz]

is example_sysid.m:22-65 (Ksysid constructor, train_models, validation of every `val` trial) with the options of
Ksysid_setup.m; prints the validation errors and optionally stores the model matrices.  With several --lasso values every
candidate is validated on every trial (one device call, Ksysid.val_candidates), the candidate with the least --metric is
chosen (Ksysid.select_model) and that one is reported and stored.  With --horizon H the choice is made by the error of the
H-th prediction step from every start sample of every trial instead (one device call, Ksysid.val_horizon), printed per
candidate.  --spectrum prints the spectral radius, stability and the
five leading eigenvalues of every candidate (one device call, Ksysid.candidate_spectra) and stores the chosen model's
eigenvalues with --out."""
from __future__ import annotations

import argparse
import sys

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(prog="koopman_realizations_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("sysid", help="fit a model to a data4sysid MAT-file and validate it")
    s.add_argument("data")
    s.add_argument("--model_type", default="linear", choices=["linear", "bilinear", "nonlinear"])
    s.add_argument("--obs_type", nargs="+", default=["poly"])
    s.add_argument("--obs_degree", nargs="+", type=int, default=[3])
    s.add_argument("--snapshots", type=float, default=float("inf"))
    s.add_argument("--lasso", nargs="+", type=float, default=[float("inf")])
    s.add_argument("--metric", default="euclid_mean", choices=["mean", "rmse", "nrmse", "euclid_mean", "unscaled_euclid_mean"],
                   help="with several --lasso values: the validation error, averaged over the trials, that picks the model")
    s.add_argument("--horizon", type=int, default=None,
                   help="choose by the --metric of the H-th prediction step from every start sample (the horizon an MPC uses), not by whole-trial rollouts")
    s.add_argument("--horizon_stride", type=int, default=1, help="with --horizon: every how many samples a prediction starts")
    s.add_argument("--delays", type=int, default=0)
    s.add_argument("--dim_red", action="store_true")
    s.add_argument("--loaded", action="store_true")
    s.add_argument("--time_type", default="discrete", choices=["discrete", "continuous"],
                   help="continuous: models of the matrix logarithm, validated by ode45 per sample interval (also one device call)")
    s.add_argument("--device", type=int, default=0)
    s.add_argument("--spectrum", action="store_true",
                   help="print radius, stability and the five leading eigenvalues of every candidate (linear / bilinear models)")
    s.add_argument("--out", default=None, help="write the model (A, B, C, K, scale) to this .npz")
    a = ap.parse_args(argv)
    if a.horizon is not None and a.metric == "nrmse":
        ap.error("--metric nrmse is not defined with --horizon")

    from . import Context, Ksysid          # needs libkoopman_hip.so and a GPU: fails loudly otherwise
    from .matio import load_data4sysid
    data = load_data4sysid(a.data)
    ctx = Context(a.device)
    ks = Ksysid(data, ctx=ctx, model_type=a.model_type, obs_type=a.obs_type, obs_degree=a.obs_degree, snapshots=a.snapshots,
                lasso=a.lasso if len(a.lasso) > 1 else a.lasso[0], delays=a.delays, dim_red=a.dim_red, loaded=a.loaded,
                time_type=a.time_type)
    ks.train_models()
    p = ks.params
    print(f"{a.model_type} {a.time_type}-time model: n={p['n']} m={p['m']} nzeta={p['nzeta']} N={p['N']}  pairs={len(ks.snapshotPairs['alpha'])}")
    tab = ks.val_candidates()               # every candidate on every trial: one device call
    many = isinstance(ks.candidates, list)

    def lines(c, indent):
        for i in range(len(ks.valdata)):
            print(f"{indent}val trial {i}: rmse {np.array2string(tab['rmse'][c, i], precision=4)}  "
                  f"nrmse {np.array2string(tab['nrmse'][c, i], precision=4)}  mean euclid {tab['euclid_mean'][c, i]:.5f}")

    if many:
        for c, lv in enumerate(tab["lasso"]):
            print(f"candidate {c}: lasso {lv:g}" + ("  (diverged)" if tab["diverged"][c].any() else ""))
            lines(c, "  ")
        if a.horizon is None:
            best, _ = ks.select_model(a.metric, tab)
            print(f"chosen by {a.metric}: candidate {best} (lasso {tab['lasso'][best]:g})")
        else:
            sl = ks.horizon_slice(ks.val_horizon(a.horizon, stride=a.horizon_stride), a.horizon)
            for c, lv in enumerate(sl["lasso"]):
                print(f"horizon {a.horizon}: candidate {c}: lasso {lv:g}  {a.metric} {sl[a.metric][c].mean():.6g}"
                      + ("  (diverged)" if sl["diverged"][c].any() else ""))
            best, _ = ks.select_model(a.metric, sl, horizon=a.horizon)
            print(f"chosen by {a.metric} at step {a.horizon}: candidate {best} (lasso {sl['lasso'][best]:g})")
    else:
        lines(0, "")
        if a.horizon is not None:
            sl = ks.horizon_slice(ks.val_horizon(a.horizon, stride=a.horizon_stride), a.horizon)
            print(f"horizon {a.horizon}: candidate 0:  {a.metric} {sl[a.metric][0].mean():.6g}" + ("  (diverged)" if sl["diverged"][0].any() else ""))
    extra = {}
    if a.spectrum and (a.model_type == "nonlinear" or a.loaded):
        print("--spectrum: not available for nonlinear or loaded models (Ksysid.spectrum covers linear and bilinear ones)")
    elif a.spectrum:
        cs = ks.candidate_spectra()         # every candidate: one device call
        for c in range(len(cs["radius"])):
            lead = "  ".join(f"{z.real:.5f}{z.imag:+.5f}j" for z in cs["lam"][c][:5])
            print(f"spectrum of candidate {c}: radius {cs['radius'][c]:.6f}  stable {bool(cs['stable'][c])}  leading {lead}")
        cands = ks.candidates if many else [ks.candidates]
        extra["lam"] = cs["lam"][[i for i, c in enumerate(cands) if c is ks.model][0]]
    if a.out:
        m = ks.model
        np.savez(a.out, **{k: np.asarray(m[k]) for k in ("A", "B", "C", "K", "Kf", "M") if k in m},
                 **{"scale_" + k: v for k, v in p["scale"].items()}, **extra)
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
