#!/usr/bin/env python3
"""Where the headline step goes, kernel by kernel, from ONE rocprofv3 kernel trace of bench.py's headline section:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --no-cpu-baseline --no-mpc --no-extras
    python3 tools/gram_step_accounting.py DIR [--steps 200 --warmup 10] [--json OUT]

bench.py issues, in this order: a queue of max(256, steps) pipelined fits, the warm-up's fits, 32 Gram-only launches, then the
timed region's `steps` fits.  Pipelined fits share a Gram launch in groups of up to kp_timer_get(12); a synchronisation, or a
full batch of deferred solves, flushes a partial group.  Every Gram launch is followed by one kp_gram3_reduce_kernel launch whose
grid's y extent is the number of fits the pair served, so the script walks the launches in start order and counts fits:
max(256, steps) of the first queue, `warmup`, the 32 Gram-only launches, then the timed region's launches until they have
served `steps` fits.

Per group launch it lists the Gram kernel, the gap to its reduction, the reduction, and the gap from the Gram kernel's end to
the next Gram kernel's start; once for the region, the solve chain: every other kernel that starts inside the region (from the
first Gram start to the last kernel that starts before the next Gram launch of the process or the end of the trace), its summed
duration, and the tail from the end of the last reduction to the end of the last such kernel.  Sums are per fit (/ steps), beside
which DESIGN 6.4 puts timers 0, 6 and 1 of the same command.  Profiler timestamps are nanoseconds.
"""
import argparse
import csv
import glob
import json
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    fs = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(fs[-1])), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    gram = [r for r in rows if "kp_gram3_kernel" in r["Kernel_Name"]]
    allred = [r for r in rows if "kp_gram3_reduce_kernel" in r["Kernel_Name"]]
    assert len(gram) == len(allred), (len(gram), len(allred))
    fits = [int(r["Grid_Size_Y"]) for r in allred]

    def skip(i, nfits):                      # index behind the launches that serve nfits fits from launch i on
        got = 0
        while got < nfits:
            got += fits[i]
            i += 1
        assert got == nfits, (got, nfits)
        return i
    first = skip(skip(0, max(256, a.steps)), a.warmup) + 32
    assert all(f == 1 for f in fits[first - 32:first]), "32 Gram-only launches in front of the timed region"
    n = skip(first, a.steps) - first
    reg = gram[first:first + n]
    t0 = reg[0]["s"]
    t_next = gram[first + n]["s"] if len(gram) > first + n else rows[-1]["e"] + 1
    inreg = [r for r in rows if t0 <= r["s"] < t_next]
    red = [r for r in inreg if "kp_gram3_reduce_kernel" in r["Kernel_Name"]]
    other = [r for r in inreg if "kp_gram3" not in r["Kernel_Name"]]
    assert len(red) == n, (len(red), n)
    per = []
    for i, g in enumerate(reg):
        per.append({"fits": fits[first + i], "gram_us": (g["e"] - g["s"]) / 1e3, "gap_to_reduce_us": (red[i]["s"] - g["e"]) / 1e3, "reduce_us": (red[i]["e"] - red[i]["s"]) / 1e3,
                    "gap_to_next_gram_us": (reg[i + 1]["s"] - g["e"]) / 1e3 if i + 1 < n else None})
    print(" group  fits   gram us  gap->reduce   reduce us  gap->next gram")
    for i, p in enumerate(per):
        print("%6d %5d %9.2f %12.2f %11.2f %15s" % (i, p["fits"], p["gram_us"], p["gap_to_reduce_us"], p["reduce_us"],
                                                 "%.2f" % p["gap_to_next_gram_us"] if p["gap_to_next_gram_us"] is not None else "-"))
    gaps = [p["gap_to_next_gram_us"] for p in per[:-1]]
    names = {}
    for r in other:
        k = r["Kernel_Name"].split("(")[0].replace("void ", "")[:48]
        c = names.setdefault(k, [0, 0.0])
        c[0] += 1
        c[1] += (r["e"] - r["s"]) / 1e3
    end_all = max(r["e"] for r in inreg)
    out = {
        "steps": a.steps, "group_launches": n, "fits_per_launch": [p["fits"] for p in per],
        "region_us": (end_all - t0) / 1e3,
        "per_fit_us": {
            "gram": sum(p["gram_us"] for p in per) / a.steps,
            "gap_gram_to_next_gram": sum(gaps) / a.steps,
            "gap_gram_to_reduce": sum(p["gap_to_reduce_us"] for p in per) / a.steps,
            "reduce": sum(p["reduce_us"] for p in per) / a.steps,
            "solve_chain_kernels": sum(v[1] for v in names.values()) / a.steps,
            "tail_after_last_reduce": (end_all - red[-1]["e"]) / 1e3 / a.steps,
            "first_gram_start_to_last_kernel_end": (end_all - t0) / 1e3 / a.steps,
        },
        "gap_to_next_gram_us": {"median": sorted(gaps)[len(gaps) // 2] if gaps else None, "min": min(gaps) if gaps else None, "max": max(gaps) if gaps else None},
        "gap_to_reduce_us": {"min": min(p["gap_to_reduce_us"] for p in per), "max": max(p["gap_to_reduce_us"] for p in per)},
        "solve_chain": {k: {"calls": v[0], "sum_us": v[1]} for k, v in sorted(names.items(), key=lambda kv: -kv[1][1])},
        "per_group": per,
    }
    print(json.dumps({k: v for k, v in out.items() if k not in ("per_group", "solve_chain")}, indent=1))
    for k, v in out["solve_chain"].items():
        print("%-50s %5d calls %10.1f us" % (k, v["calls"], v["sum_us"]))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
