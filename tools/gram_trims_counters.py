#!/usr/bin/env python3
"""Instruction counters of the pipelined Gram kernel per fit: 16 pipelined fits of the headline dictionary at 1e5 pairs.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_INSTS_LDS --output-format csv -d DIR -- python3 tools/gram_trims_counters.py
    python3 tools/gram_trims_counters.py DIR          (prints one JSON line: every counter summed over the kp_gram3_kernel launches / 16)

A counter run of its own, no tracing.  KP_LIB_PATH selects another build of the library (the parent's, for A/B)."""
import csv
import glob
import json
import os
import sys

FITS = 16
if len(sys.argv) > 1:
    acc, launches = {}, 0
    for f in glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True):
        seen = set()
        for r in csv.DictReader(open(f)):
            if "kp_gram3_kernel" in r["Kernel_Name"]:
                acc[r["Counter_Name"]] = acc.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                seen.add(r["Dispatch_Id"])
        launches += len(seen)
    out = {k + "_per_fit": v / FITS for k, v in sorted(acc.items())}
    out["launches"] = launches
    if "SQ_INSTS_VALU_per_fit" in out and "SQ_INSTS_VALU_MFMA_MOPS_F64_per_fit" in out:
        out["non_mfma_valu_per_fit"] = out["SQ_INSTS_VALU_per_fit"] - out["SQ_INSTS_VALU_MFMA_MOPS_F64_per_fit"]
    print(json.dumps(out))
    sys.exit(0)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import koopman_realizations_amd as kra
import bench

ctx = kra.Context(0)
a, b, u = (np.asfortranarray(x) for x in bench.synth_pairs(100000))
basis = kra.Basis(ctx, "bilinear", 6, 3, [("poly", kra.poly_exponent_table(6, 3)[6:])])
snaps = kra.Snapshots(ctx, a, b, u)
ctx.fit_async_slots(FITS)
for _ in range(FITS):
    kra.fit(ctx, basis, snaps, fetch=False)
ctx.synchronize()
print("fits", FITS, "timer10", ctx.timer(10), "timer15", ctx.timer(15))
