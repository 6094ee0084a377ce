#!/usr/bin/env python3
"""Condenses the alternating A/B runs of the two tile-loop trims into profiles/gram_trims_ab.json:

    python3 tools/gram_trims_ab_summarize.py DIR [OUT]

DIR holds one bench.py JSON line per run, <mode>_<variant>_<i>.json (mode: default = `python bench.py`, driver = `python bench.py
--gpus 1 --steps 20 --warmup 5`; variant: parent = the parent commit's library, t1 = lift slots ordered by factor count alone,
t2 = three-entry power table alone, both), and <mode>_<variant>_<i>.ksha, the first 16 hex digits of the SHA-256 of the K that
run dumped (--dump-outputs), and <mode>_<variant>_<i>.err, its stderr with the detail line.  Per mode and variant: median, min, max and every value of the figures of DESIGN 6.4, and whether a
variant's ms_per_step range lies wholly below the parent's."""
import glob
import json
import os
import sys

FIELDS = {
    "ms_per_step": lambda d: d["ms_per_step"],
    "value": lambda d: d["value"],
    "gram_ms": lambda d: d["kernel_ms"]["gram"],
    "gram_reduce_ms": lambda d: d["kernel_ms"]["gram_reduce"],
    "solve_ms": lambda d: d["kernel_ms"]["solve"],
    "roofline_frac": lambda d: d["roofline"]["frac"],
    "fit_latency_ms": lambda d: d["fit_latency_ms"],
    "points.Ns11999.gram_ms": lambda d: d["points"]["Ns11999"][0],
    "points.Ns11999.ms_per_fit": lambda d: d["points"]["Ns11999"][2],
    "points.Ns1000000.gram_ms": lambda d: d["points"]["Ns1000000"][0],
    "points.Ns1000000.ms_per_fit": lambda d: d["points"]["Ns1000000"][2],
    "points.Ns10000000.gram_ms": lambda d: d["points"]["Ns10000000"][0],
    "points.Ns10000000.ms_per_fit": lambda d: d["points"]["Ns10000000"][2],
    "points.W200.gram_ms": lambda d: d["points"]["W200"][0],
}


def find(d, key):
    if isinstance(d, dict):
        if key in d:
            return d[key]
        for v in d.values():
            r = find(v, key)
            if r is not None:
                return r
    return None


def main():
    src = sys.argv[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "gram_trims_ab.json")
    out = {"what": "alternating full runs of bench.py on one MI355X, one session per command, order parent, t1, t2, both, five times: the parent "
                   "commit's library (parent); lift slots ordered by factor count with two-factor lift steps alone (t1); the three-entry power "
                   "table alone (t2: what this commit keeps); both trims (both).  tools/gram_trims_ab_summarize.py",
           "commands": {"default": "python bench.py", "driver": "python bench.py --gpus 1 --steps 20 --warmup 5"}}
    for mode in ("default", "driver"):
        sec = {}
        for v in ("parent", "t1", "t2", "both"):
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
            for f in files:                    # bench.py's detail line (stderr, kept as .err) holds the spread of K over the timed region
                det = [l for l in open(f[:-5] + ".err") if l.startswith("{")] if os.path.exists(f[:-5] + ".err") else []
                spread.append(find(json.loads(det[-1]), "K_first_vs_last_max_abs_diff") if det else None)
            e["K_first_vs_last_max_abs_diff"] = spread
            e["K_sha256_16"] = sorted({open(f[:-5] + ".ksha").read().strip() for f in files if os.path.exists(f[:-5] + ".ksha")})
            sec[v] = e
        if "parent" in sec:
            p = sec["parent"]["ms_per_step"]
            for v in ("t1", "t2", "both"):
                if v in sec:
                    c = sec[v]["ms_per_step"]
                    sec[v]["ms_per_step_range_below_parent"] = c["max"] < p["min"]
                    sec[v]["ms_per_step_range_above_parent"] = c["min"] > p["max"]
                    sec[v]["ms_per_step_change_percent"] = round(100.0 * (c["median"] / p["median"] - 1.0), 2)
            sec["K_bitwise_equal_across_variants"] = len({s for v in sec.values() if isinstance(v, dict) for s in v.get("K_sha256_16", [])}) == 1
        out["full_" + mode] = sec
    prev = json.load(open(dst)) if os.path.exists(dst) else {}
    for k in ("counters", "kernel_text", "accounting"):
        if k in prev:
            out[k] = prev[k]
    json.dump(out, open(dst, "w"), indent=1)
    for mode in ("default", "driver"):
        for v, e in out.get("full_" + mode, {}).items():
            if isinstance(e, dict):
                print(mode, v, {k: (round(e[k]["median"], 6), round(e[k]["min"], 6), round(e[k]["max"], 6)) for k in ("ms_per_step", "gram_ms")},
                      e.get("ms_per_step_range_below_parent"), e.get("ms_per_step_change_percent"))


if __name__ == "__main__":
    main()
