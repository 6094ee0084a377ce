"""Time of the validation table: ONE Ksysid.val_candidates call (kp_validate: models and trials uploaded once, one launch,
errors reduced on the device) against the loop it replaces, one val_model / val_BLmodel / val_NLmodel call per (candidate,
trial) pair - host lift, uploads, a launch, the trajectory copied back and get_error on the host, each time.  Same process,
best of 5 after a warm-up, host clock around calls that end in a device synchronise.

Shapes: the arm data (tests/golden/arm_data.npz: n = 6, m = 3), poly-3 dim_red dictionaries, linear / bilinear / nonlinear,
16 candidates x 5 validation trials = 80 pairs.  The stored file holds one validation trial (401 rows), so the last four
of its ten training trials (1201 rows each) are held out as the other four; the 16 candidates are least-squares fits on 16
snapshot counts (what is timed does not depend on how a candidate was fitted).
Then the toy loaded system (tests/_loaded_system.py, nw = 2) with a load that changes at every step - a random walk inside
[-1, 1] - where the per-trial route launches once per sample: one model on the two validation trials of 150 rows.
Then the same arm shape with time_type = 'continuous' (kp_validate_ct against the loop of kp_rollout_ct / kp_rollout_nl_ct
calls, ode45 over every sample interval): the 16 candidates are the trained continuous model with its matrix scaled by
1 + i / 1000, since the matrix logarithm of a fit on a subset of the pairs need not exist.
Prints one JSON line per configuration, and the largest difference between the two routes' euclid_mean.
Usage: validate_time.py [all | discrete | continuous]."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import koopman_realizations_amd as kra  # noqa: E402
from koopman_realizations_amd import _ffi as F  # noqa: E402
from tests._loaded_system import make_trials  # noqa: E402


def best_of(fn, reps=5):
    fn()                                                                   # warm-up: workspaces, code objects
    best = np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return best, out


def candidates(ks, counts):
    extract = {"nonlinear": ks.get_NLmodel, "bilinear": ks.get_BLmodel, "linear": ks.get_model}[ks.model_type]
    out = []
    for cnt in counts:
        sub = {k: F.fcol(np.asarray(x)[:cnt]) for k, x in ks.snapshotPairs.items()}
        kd = ks.get_Koopman(sub)
        kd["beta"] = sub["beta"]
        out.append(extract(kd))
    return out


def compare(ks, cands, trials, label):
    val = {"linear": ks.val_model, "bilinear": ks.val_BLmodel, "nonlinear": ks.val_NLmodel}[ks.model_type]
    t_loop, res = best_of(lambda: [[val(mo, v)["error"]["euclid_mean"] for v in trials] for mo in cands])
    t_one, tab = best_of(lambda: ks.val_candidates(cands, trials))
    with np.errstate(invalid="ignore"):
        diff = float(np.nanmax(np.abs(np.array(res) - tab["euclid_mean"])))
    print(json.dumps({"case": label, "model_type": ks.model_type, "N": ks.params["N"], "pairs": len(cands) * len(trials),
                      "rows": int(sum(len(np.ravel(v["t"])) for v in trials)), "loop_ms": round(t_loop * 1e3, 3),
                      "val_candidates_ms": round(t_one * 1e3, 3), "kernel_ms": round(ks.ctx.timer(5), 3),
                      "ratio": round(t_loop / t_one, 1), "diverged": int(tab["diverged"].sum()), "max_diff_euclid_mean": diff}), flush=True)


def scaled_candidates(ks, count):
    key = "Kf" if ks.model_type == "nonlinear" else "A"
    return [dict(ks.model, **{key: np.asfortranarray(ks.model[key] * (1.0 + 1e-3 * i))}) for i in range(count)]


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which not in ("all", "discrete", "continuous"):
        raise SystemExit(__doc__)
    g = np.load(os.path.join(ROOT, "tests", "golden", "arm_data.npz"))
    off = np.concatenate([[0], np.cumsum(g["train_len"])])
    runs = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}] + runs[6:]
    ctx = kra.Context(0)
    for mt in ("linear", "bilinear", "nonlinear") if which != "continuous" else ():
        ks = kra.Ksysid({"train": runs[:6], "val": val}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[3], dim_red=True)
        npairs = len(ks.snapshotPairs["alpha"])
        cands = candidates(ks, np.linspace(npairs // 2, npairs, 16).astype(int))
        compare(ks, cands, ks.valdata, "arm 16 x 5")
    for mt in ("linear", "bilinear", "nonlinear") if which != "discrete" else ():
        ks = kra.Ksysid({"train": runs[:6], "val": val}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[3], dim_red=True,
                        time_type="continuous")
        ks.train_models()
        compare(ks, scaled_candidates(ks, 16), ks.valdata, "arm 16 x 5, continuous")
    rng = np.random.default_rng(3)
    trials = make_trials(10, 150, nw=2, seed=21)
    for mt in ("linear", "bilinear", "nonlinear") if which != "continuous" else ():
        ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[2], loaded=True)
        ks.train_models()
        walk = []
        for v in ks.valdata:
            w = np.clip(v["w"][0] + np.cumsum(rng.uniform(-0.1, 0.1, v["w"].shape), axis=0), -1.0, 1.0)
            walk.append(dict(v, w=w))
        compare(ks, [ks.model], walk, "loaded toy, nw = 2, load changes every step")
    ctx.close()


if __name__ == "__main__":
    main()
