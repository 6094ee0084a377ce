"""Time of prediction-horizon validation: ONE Ksysid.val_horizon call (kp_validate_horizon: the h-step-ahead errors, h = 1 .. H,
of every candidate from every start sample of every validation trial) against two host routes.

Data: the arm data (tests/golden/arm_data.npz: n = 6, m = 3), poly-3 dim_red dictionaries, 16 candidates x 5 validation trials,
built as tools/validate_time.py builds them.  Cases: H = 10 and 50, stride 1; linear, bilinear, nonlinear.  Best of 5 after a
warm-up, host clock around calls that end in a device synchronise.
  device    the whole val_horizon call, and its two kernels' own time (kp_timer_get(24)); the tile width and whether the model
            rows were staged (kp_timer_get(25))
  numpy     tests/_horizon_reference.py on the same machine: one matrix product per step over all starts of a trial - the fair
            host baseline (a pass of more than 10 s is timed once; numpy_reps says which)
  loop      one Context.rollout / rollout_nl call per (candidate, start), timed on 64 starts of the first candidate and trial
            and SCALED to the start count: not measured in full
Kernel figures: the flop of the f64 MFMAs it executes (512 per v_mfma_f64_4x4x4_4b: padded rows, padded contraction, unused
columns of a trial's last tile included), the flop of the definition (2 R K per start and step, and 2 k_pcs nfull for a nonlinear
dim_red lift), and the executed flop per second as a fraction of the 78.6 TFLOP/s f64 matrix peak.
Writes profiles/horizon_time.json and prints the rows of the README table."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import koopman_realizations_amd as kra  # noqa: E402
from koopman_realizations_amd import _ffi as F  # noqa: E402
from oracle import koopman_oracle as ko  # noqa: E402
from tests import _horizon_reference as hr  # noqa: E402

PEAK = 78.6e12


def best_of(fn, reps=5):
    fn()
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


def pad4(x):
    return (x + 3) // 4 * 4


def flops(ks, starts, nmod, H, ST):
    """(executed on the matrix pipe, of the definition) for the whole call."""
    p = ks.params; N, m, nz = p["N"], p["m"], p["nzeta"]
    b = ks.basis_dev
    nl = ks.model_type == "nonlinear"
    K = {"linear": N + m, "bilinear": N * (1 + m), "nonlinear": N}[ks.model_type]
    R = nz if nl else N
    kp = b.N - b.nvars - 1 if ks.dim_red else 0
    mfma = (pad4(R) // 4) * (pad4(K) // 4)                          # per 16 columns and step
    lift = (pad4(kp) // 4) * (pad4(b.nfull) // 4) if kp else 0      # pcs' full
    tiles = sum(-(-int(s) // ST) for s in starts)
    per_tile = (ST // 16) * (H * mfma + (H if nl else 1) * lift)
    useful = nmod * int(np.sum(starts)) * (H * 2 * R * K + (H if nl else 1) * 2 * kp * b.nfull)
    return 512.0 * nmod * tiles * per_tile, float(useful)


def case(ks, cands, H):
    mt, p = ks.model_type, ks.params
    t_dev, tab = best_of(lambda: ks.val_horizon(H, cands))
    kern = ks.ctx.timer(F.TIMER_HORIZON)
    code = int(ks.ctx.timer(F.TIMER_HORIZON_TILE))
    ST, staged = code % 1000, code // 1000
    dic = ko.build_dictionary(mt, p["nzeta"], p["m"], ["poly"], [3])
    dic.pcs = np.asarray(ks.basis["pcs"], dtype=np.float64)
    zu = [(ks._val_common(v)[3], ks._val_common(v)[2]) for v in ks.valdata]
    t0 = time.perf_counter()
    ref, _ = hr.horizon_table(dic, cands, zu, p["n"], p["scale"]["y_factor"], H)
    t_np, np_reps = time.perf_counter() - t0, 1
    if t_np < 10.0:                                                  # a pass of more than 10 s is timed once, and the row says so
        t_np, np_reps = best_of(lambda: hr.horizon_table(dic, cands, zu, p["n"], p["scale"]["y_factor"], H))[0], 5
    with np.errstate(invalid="ignore"):
        diff = float(np.nanmax(np.abs(ref["euclid_mean"] - tab["euclid_mean"])))
    Z, U = zu[0]
    mo = cands[0]
    if mt == "nonlinear":
        one = lambda s: ks.ctx.rollout_nl(ks.basis_dev, mo["Kf"], Z[s], U[s:s + H + 1])
    else:
        one = lambda s: ks.ctx.rollout(mt, mo["A"], mo["B"], ks.lift.econ_full(Z[s]), U[s:s + H + 1], p["n"])
    t64, _ = best_of(lambda: [one(s) for s in range(64)])
    total = len(cands) * int(tab["starts"].sum())
    ex, useful = flops(ks, tab["starts"], len(cands), H, ST)
    row = {"model_type": mt, "N": p["N"], "H": H, "stride": 1, "candidates": len(cands), "trials": len(zu), "starts": total,
           "tile": ST, "staged": staged, "val_horizon_ms": round(t_dev * 1e3, 3), "kernel_ms": round(kern, 4),
           "numpy_ms": round(t_np * 1e3, 1), "numpy_reps": np_reps, "loop_64_starts_ms": round(t64 * 1e3, 2), "loop_scaled_ms": round(t64 * 1e3 * total / 64.0, 0),
           "flop_executed": ex, "flop_definition": useful, "tflops_executed": round(ex / (kern * 1e-3) / 1e12, 3),
           "peak_fraction": round(ex / (kern * 1e-3) / PEAK, 4), "diverged": int(tab["diverged"].sum()), "max_diff_euclid_mean": diff}
    print(json.dumps(row), flush=True)
    return row


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "arm_data.npz"))
    off = np.concatenate([[0], np.cumsum(g["train_len"])])
    runs = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}] + runs[6:]
    ctx = kra.Context(0)
    rows = []
    for mt in ("linear", "bilinear", "nonlinear"):
        ks = kra.Ksysid({"train": runs[:6], "val": val}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[3], dim_red=True)
        npairs = len(ks.snapshotPairs["alpha"])
        cands = candidates(ks, np.linspace(npairs // 2, npairs, 16).astype(int))
        for H in (10, 50):
            rows.append(case(ks, cands, H))
    ctx.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "horizon_time.json"), "w") as f:
        json.dump({"device": "MI355X", "reps": 5, "peak_f64_matrix_flops": PEAK, "rows": rows}, f, indent=1)
    print("| shape | H | starts | numpy restatement | loop of rollout calls (64 starts, scaled) | one `val_horizon` call | kernels | executed / definition GFLOP | of f64 matrix peak |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| arm, {r['model_type']} (N = {r['N']}), 16 x 5, S_T = {r['tile']} | {r['H']} | {r['starts']} | {r['numpy_ms']:.0f} ms | "
              f"{r['loop_scaled_ms']:.0f} ms | {r['val_horizon_ms']:.2f} ms | {r['kernel_ms']:.3f} ms | "
              f"{r['flop_executed'] / 1e9:.2f} / {r['flop_definition'] / 1e9:.2f} | {100 * r['peak_fraction']:.2f} % |")


if __name__ == "__main__":
    main()
