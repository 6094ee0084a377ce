"""Windows per second of the batched load observer (Ksysid.val_observer_load on the device: one kp_load_observe call for
all windows of all trials) against the host route, a Python loop of Kmpc.estimate_load_* calls (host-assembled rows,
one device QP per window).  Trials of 1 000 samples, 1 / 8 / 64 trials, hor = 11 and 101, on the toy loaded system
(poly degree 2: N = 6) and on a wider dictionary (poly degree 6: N = 28).  Prints one JSON line per configuration."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import koopman_realizations_amd as kra  # noqa: E402
from tests._loaded_system import make_trials  # noqa: E402


def main():
    T = 1000
    for deg in (2, 6):
        train = make_trials(8, 150, nw=1, seed=7)
        ks = kra.Ksysid({"train": train, "val": train[:1]}, model_type="bilinear", obs_type=["poly"], obs_degree=[deg],
                        loaded=True)
        ks.train_models()
        mpc = kra.Kmpc(ks, horizon=8)
        runs = [ks.scale_data(v) for v in make_trials(64, T, nw=1, seed=11)]
        for hor in (11, 101):
            # host route: estimate_load_bilinear per window over the first trial (200 windows are enough for a rate)
            v = runs[0]
            t0 = time.perf_counter()
            nh = 200
            for i in range(hor, hor + nh):
                mpc.estimate_load_bilinear(v["y"][i - hor:i], v["u"][i - hor:i])
            host_rate = nh / (time.perf_counter() - t0)
            for ntr in (1, 8, 64):
                trials = runs[:ntr]
                ks.val_observer_load(hor, trials)                          # warm-up (workspace, code objects)
                reps = 5
                t0 = time.perf_counter()
                for _ in range(reps):
                    ks.val_observer_load(hor, trials)
                dt = (time.perf_counter() - t0) / reps
                nwin = ntr * (T - 1)
                print(json.dumps({"N": ks.params["N"], "hor": hor, "trials": ntr, "windows": nwin,
                                  "device_windows_per_s": round(nwin / dt), "device_ms_per_call": round(dt * 1e3, 3),
                                  "kernel_ms": round(ks.ctx.timer(4), 3), "host_route_windows_per_s": round(host_rate, 1)}),
                      flush=True)


if __name__ == "__main__":
    main()
