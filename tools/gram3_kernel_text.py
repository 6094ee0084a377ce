#!/usr/bin/env python3
"""Instruction counts of one kp_gram3_kernel instantiation from the compiler's text (the register table of DESIGN 6.7 / 6.8):

    hipcc -S --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -Iinclude -I<csrc> <csrc>/kp_gram3.hip -o kp_gram3.s
    python3 tools/gram3_kernel_text.py kp_gram3.s 6 3 0 0 0 1 1 1

The arguments behind the file are the template arguments NQ BM PCS EXT PRE P3 LO EB (a text from before HISTORY.md's "Opt-in forms
of the Kronecker Gram kernel" has TUP behind PRE; one from before the early barrier no EB).  Prints one JSON line: v_mfma, v_mul_f64, ds_read*, ds_write*, scratch_*, s_barrier in the whole instantiation; VGPRs
and scratch bytes from the kernel descriptor's comments; and per tile loop (a backward branch whose body holds MFMAs) the
number of tile bodies' worth of MFMAs, of vector instructions (MFMAs included) and of scratch accesses in it."""
import json
import re
import sys


def main():
    text, args = sys.argv[1], sys.argv[2:]
    mangled = "_Z15kp_gram3_kernelILi%sELi%s%sEEv9Gram3Args" % (args[0], args[1], "".join("ELb%s" % a for a in args[2:]))
    body, on = [], False
    for line in open(text):
        if line.startswith(mangled + ":"):
            on = True
            continue
        if on:
            if line.startswith(".Lfunc_end"):
                break
            body.append(line.strip())
    if not body:
        sys.exit("no such instantiation: " + mangled)
    ins = [l.split()[0] for l in body if l and not l.startswith((";", ".", "/")) and not l.endswith(":")]
    count = lambda p: sum(1 for i in ins if i.startswith(p))
    out = {"kernel": mangled, "v_mfma": count("v_mfma"), "v_mul_f64": count("v_mul_f64"), "ds_read": count("ds_read"), "ds_write": count("ds_write"),
           "scratch": count("scratch_"), "s_barrier": count("s_barrier")}
    whole = open(text).read()
    meta = whole[whole.index(".Lfunc_end", whole.index("\n" + mangled + ":")):]
    for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"), ("scratch_bytes", r"; ScratchSize: (\d+)"), ("sgprs", r"; NumSgprs: (\d+)"),
                     ("occupancy", r"; Occupancy: (\d+)")):
        m = re.search(pat, meta)
        out[key] = int(m.group(1)) if m else None
    # tile loops: the strongly connected components of the control-flow graph (blocks = labels, edges = branches and fall-through) that hold MFMAs
    blocks, cur = {"entry": []}, "entry"
    order = ["entry"]
    for l in body:
        lab = re.match(r"(\.LBB\w+):", l)               # (a loop header's label carries a comment behind the colon)
        if lab:
            cur = lab.group(1)
            blocks[cur] = []
            order.append(cur)
        elif l and not l.startswith((";", ".", "/")):
            blocks[cur].append(l)
    succ = {}
    for i, name in enumerate(order):
        out_edges, fall = [], True
        for l in blocks[name]:
            m = re.match(r"s_(c?)branch\w*\s+(\.LBB\w+)", l)
            if m:
                out_edges.append(m.group(2))
                if not m.group(1):
                    fall = False
            elif l.startswith(("s_endpgm", "s_setpc")):
                fall = False
        if fall and i + 1 < len(order):
            out_edges.append(order[i + 1])
        succ[name] = [e for e in out_edges if e in blocks]
    index, low, stack, on_stack, sccs, counter = {}, {}, [], set(), [], [0]
    sys.setrecursionlimit(100000)

    def visit(v):
        index[v] = low[v] = counter[0]
        counter[0] += 1
        stack.append(v)
        on_stack.add(v)
        for w in succ[v]:
            if w not in index:
                visit(w)
                low[v] = min(low[v], low[w])
            elif w in on_stack:
                low[v] = min(low[v], index[w])
        if low[v] == index[v]:
            comp = []
            while True:
                w = stack.pop()
                on_stack.discard(w)
                comp.append(w)
                if w == v:
                    break
            if len(comp) > 1 or v in succ[v]:
                sccs.append(comp)
    for v in order:
        if v not in index:
            visit(v)
    loops = []
    for comp in sccs:
        seg = [l.split()[0] for name in comp for l in blocks[name]]
        nm = sum(1 for x in seg if x.startswith("v_mfma"))
        if nm:
            loops.append({"first_block": min(comp, key=order.index), "v_mfma": nm, "vector": sum(1 for x in seg if x.startswith("v_")),
                          "v_mul_f64": sum(1 for x in seg if x.startswith("v_mul_f64")), "scratch": sum(1 for x in seg if x.startswith("scratch_")),
                          "ds_read": sum(1 for x in seg if x.startswith("ds_read")), "ds_write": sum(1 for x in seg if x.startswith("ds_write")),
                          "s_barrier": sum(1 for x in seg if x.startswith("s_barrier")), "s_waitcnt": sum(1 for x in seg if x.startswith("s_waitcnt"))})
    loops.sort(key=lambda e: order.index(e["first_block"]))
    out["tile_loops"] = loops
    print(json.dumps(out))


if __name__ == "__main__":
    main()
