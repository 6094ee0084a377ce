#!/usr/bin/env python3
"""Condenses the alternating A/B runs of the early tile barrier into profiles/gram_early_barrier_ab.json:

    python3 tools/gram_early_barrier_ab_summarize.py DIR SESSION [OUT]

DIR holds one bench.py JSON line per run, <mode>_<variant>_<i>.json (mode: default = `python bench.py`, driver = `python bench.py
--gpus 1 --steps 20 --warmup 5`; variant: parent = the parent commit's library through KP_LIB_PATH, change = this commit's - the
barrier at the end of step NSTEP - 1 - PF, lift chunks three steps apart -, cand2 = the second placement, today's lift timing
and the barrier behind step NSTEP - 2, a build with -DKP_GRAM3_EB_BEHIND=1), <mode>_<variant>_<i>.ksha_full, the SHA-256 of the K
that run dumped (--dump-outputs), and <mode>_<variant>_<i>.err, its stderr with the detail line.  Per mode and variant: median,
min, max and every value of the figures of DESIGN 6.8, and whether a variant's ms_per_step range lies wholly below the parent's
(the rule of DESIGN 6.4).  Every other section of an existing OUT ("counters", "kernel_text", "kernel_trace") is kept.  (Same
layout as tools/gram_lift_order_ab_summarize.py, which knows two variants only.)"""
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gram_trims_ab_summarize import FIELDS, find          # noqa: E402

VARIANTS = ("parent", "change", "cand2")


def main():
    src = sys.argv[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    session = sys.argv[2]
    dst = sys.argv[3] if len(sys.argv) > 3 else os.path.join(root, "profiles", "gram_early_barrier_ab.json")
    prev = json.load(open(dst)) if os.path.exists(dst) else {}
    top = {"what": "alternating full runs of bench.py on one MI355X, order parent, change, cand2, per command: the parent commit's library "
                   "(parent) against this commit's (change: tile barrier at the end of quad step NSTEP - 1 - PF, DESIGN 6.8) and the second "
                   "placement (cand2: barrier behind step NSTEP - 2, today's lift timing).  tools/gram_early_barrier_ab_summarize.py",
           "commands": {"default": "python bench.py", "driver": "python bench.py --gpus 1 --steps 20 --warmup 5"}}
    for k, v in prev.items():
        if k not in top:
            top[k] = v
    out = {}
    for mode in ("default", "driver"):
        sec = {}
        for v in VARIANTS:
            files = sorted(glob.glob(os.path.join(src, "%s_%s_[0-9]*.json" % (mode, v))))
            if not files:
                continue
            runs = [json.load(open(f)) for f in files]
            e = {"runs": len(runs)}
            for name, get in FIELDS.items():
                try:
                    vals = [float(get(d)) for d in runs]
                except (KeyError, TypeError, IndexError):
                    continue
                e[name] = {"median": sorted(vals)[len(vals) // 2], "min": min(vals), "max": max(vals), "all": vals}
            spread = []
            for f in files:
                det = [l for l in open(f[:-5] + ".err") if l.startswith("{")] if os.path.exists(f[:-5] + ".err") else []
                spread.append(find(json.loads(det[-1]), "K_first_vs_last_max_abs_diff") if det else None)
            e["K_first_vs_last_max_abs_diff"] = spread
            e["K_sha256"] = sorted({open(f[:-5] + ".ksha_full").read().strip() for f in files if os.path.exists(f[:-5] + ".ksha_full")})
            sec[v] = e
        if "parent" in sec:
            p = sec["parent"]["ms_per_step"]
            for v in VARIANTS[1:]:
                if v in sec:
                    c = sec[v]["ms_per_step"]
                    sec[v]["ms_per_step_range_below_parent"] = c["max"] < p["min"]
                    sec[v]["ms_per_step_range_above_parent"] = c["min"] > p["max"]
                    sec[v]["ms_per_step_change_percent"] = round(100.0 * (c["median"] / p["median"] - 1.0), 2)
            sec["K_bitwise_equal_across_variants"] = len({s for v in VARIANTS if v in sec for s in sec[v]["K_sha256"]}) == 1
        out["full_" + mode] = sec
    top[session] = out
    json.dump(top, open(dst, "w"), indent=1)
    for mode in ("default", "driver"):
        for v, e in out.get("full_" + mode, {}).items():
            if isinstance(e, dict):
                print(mode, v, {k: (round(e[k]["median"], 6), round(e[k]["min"], 6), round(e[k]["max"], 6)) for k in FIELDS if k in e},
                      e.get("ms_per_step_range_below_parent"), e.get("ms_per_step_change_percent"), e.get("K_sha256"), e.get("K_first_vs_last_max_abs_diff"))


if __name__ == "__main__":
    main()
