"""GPU tests of the Kronecker Gram kernel's early tile barrier (kp_gram3.hip: the EB form of the in-kernel-lift monomial kernel,
gram3_tile_timing).  The tile's workgroup barrier sits at the end of quad step NSTEP - 1 - PF instead of behind the last step, the
lift's three chunks finish in front of it, and the tile's last steps request the next tile's first operands from the other Psi
buffer.  The instructions and every accumulator's order are the same, so G, C and K must be the SAME BITS as with
KP_GRAM3_EARLY_BARRIER=0, which keeps the barrier behind the last step everywhere.

KP_GRAM3_EARLY_BARRIER (and KP_GRAM3_NQ, the tuning override of quads per wave) are read once, hence fresh interpreters, in
pairs: the default and KP_GRAM3_EARLY_BARRIER=0, each with KP_GRAM3_NQ unset, 4 and 5.  kra.fit_gram runs the circulant plan (a
lone launch), the queues of pipelined fits the dictionary's cover / one-A-group plan in lone and grouped launches - every launch
form of the kernel.  The children compute, this process compares.

Dictionaries (all bilinear).  kp_timer_get(26) = 1 where the last Gram launch had the early barrier: the ordered lift
(kp_timer_get(20) = 1; B operands PF = 2 steps ahead) with NQ >= 4 quads per wave (NSTEP = 2 NQ quad steps per tile: the lift's
last store must lie at or before step NSTEP - 1 - PF with chunks at least two steps apart), and at NQ = 6 with three inputs only a
plan without jobs of two A groups (kp_timer_get(15) = 0; DESIGN 6.8: the register table) - _early_expected below.  By KP_GRAM3_NQ
unset / 4 / 5, lone launch of the circulant plan | queued fits on the cover / one-A-group plan:
  headline   6 states, 3 inputs, poly-3: N = 84, W = 336, NQ = 6, ordered lift                          0 | 1,  1 | 1,  1 | 1
  head_m2    the same columns, 2 inputs: W = 252, NQ = 6, ordered lift                                  1 | 1
  poly2_m1   3 states, 1 input, poly-2: N = 10, W = 20: two quads per A group, NQ <= 2                  0 | 0   (today's placement)
  xyz80      6 states, 3 inputs: the states, the 80 monomials of degree 3 and 4 in exactly three variables, the
             constant: N = 87, W = 348, NQ = 6, the order e = tid + 256 j                               0 | 0,  0 | 0,  0 | 0
Snapshot counts and the tiles per workgroup (nkt) they produce in a lone launch of the headline, whose one-A-group plan has 73
splits and whose circulant plan 85 (tiles = ceil(Ns / 8), kps = ceil(tiles / min(tiles, splits)), ceil(tiles / kps) workgroup
rows are launched, the last one with the remainder):
  Ns = 5      1 tile, partial            73: nkt 1             85: nkt 1
  Ns = 12     2 tiles                    73: 1, 1              85: 1, 1
  Ns = 61     8 tiles                    73: 1 x 8             85: 1 x 8
  Ns = 1100   138 tiles, last partial    73: 2 x 69            85: 2 x 69         (an even number of tiles in every workgroup)
  Ns = 1597   200 tiles, last partial    73: 3 x 66, 2         85: 3 x 66, 2
  Ns = 4099   513 tiles, last partial    73: 8 x 64, 1         85: 7 x 73, 2
  grouped launches of G = 5 fits (14 splits each) at Ns = 4099: 37 x 13, 32; at Ns = 1597: 15 x 13, 5; at 1100: 10 x 13, 8
so nkt = 1, 2, 3, odd > 3 and even > 3 all occur, as the peeled first tile, inside the loop of two and as its remainder.  nkt = 0
cannot: the launcher starts no workgroup row behind the last tile (gram3_launch_n: nsplit = ceil(tiles / kps)), with fewer tiles
than splits it starts one row per tile.

Tolerances: bitwise equality between the children (np.array_equal).  Against the oracle's dense products at Ns = 4099: 1e-12
max|G| (tests/test_gpu_fit_cover.py).  K is only defined while the Gram matrix is positive definite, W < Ns: queues of 1, G and
G + 1 pipelined fits (G = kp_timer_get(12)).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_realizations_amd as kra
from conftest import synth_pairs
from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSS = (5, 12, 61, 1100, 1597, 4099)
SEED = 131
TIMER_EB = 26


def _exactly_three_variables(nz, deg):
    t = kra.poly_exponent_table(nz, deg)[nz:]
    return t[(t > 0).sum(axis=1) == 3]


# name: (states, inputs, exponent rows of the poly block, W, quads per wave by KP_GRAM3_NQ (None: unset; 0: the plan's own small count),
#        kp_timer_get(26) expected of the queued fits by KP_GRAM3_NQ)
DICTS = {
    "headline": (6, 3, lambda: kra.poly_exponent_table(6, 3)[6:], 336, {None: 6, 4: 4, 5: 5}, {None: 1, 4: 1, 5: 1}),
    "head_m2": (6, 2, lambda: kra.poly_exponent_table(6, 3)[6:], 252, {None: 6}, {None: 1}),
    "poly2_m1": (3, 1, lambda: kra.poly_exponent_table(3, 2)[3:], 20, {None: 0}, {None: 0}),
    "xyz80": (6, 3, lambda: _exactly_three_variables(6, 4), 348, {None: 6, 4: 4, 5: 5}, {None: 0, 4: 0, 5: 0}),
}


def _early_expected(name, nq, t):
    """The launcher's rule (gram3_launch_n), from the timers of the same launch: t = timers 10, 16, 20, 26, 15."""
    quads, m = DICTS[name][4][nq], DICTS[name][1]
    return float(t[2] == 1.0 and quads >= 4 and (t[4] == 0.0 or quads < 6 or m < 3))


NQS = (None, 4, 5)
CASES = [(nq, name) for nq in NQS for name in DICTS if nq in DICTS[name][4]]

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from conftest import synth_pairs
from test_gpu_fit_early_barrier import DICTS, NSS, SEED, TIMER_EB
out = sys.argv[2]
nq = int(sys.argv[3]) if sys.argv[3] != "None" else None
ctx = kra.Context(0)
grp = int(ctx.timer(12))
res = {"group": np.int64(grp)}
for name, (nz, m, exps, W, want, _) in DICTS.items():
    if nq not in want:
        continue
    b = kra.Basis(ctx, "bilinear", nz, m, [("poly", exps())])
    assert b.W == W, (name, b.W)
    for Ns in NSS:
        key = "%s_%d" % (name, Ns)
        pairs = [synth_pairs(Ns, nz, m, seed=SEED + i) for i in range(grp + 1)]
        snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in pairs]
        G, C = kra.fit_gram(ctx, b, snaps[0])
        res["G_" + key], res["C_" + key] = G, C
        res["t_" + key] = np.array([ctx.timer(10), ctx.timer(16), ctx.timer(20), ctx.timer(TIMER_EB), ctx.timer(15)])
        if not W < Ns:
            continue
        for n in sorted({1, grp, grp + 1}):
            for i in range(n):
                kra.fit(ctx, b, snaps[i], fetch=False)
            ctx.synchronize()
            res["tq%d_%s" % (n, key)] = np.array([ctx.timer(10), ctx.timer(16), ctx.timer(20), ctx.timer(TIMER_EB), ctx.timer(15)])
            res["Kq%d_%s" % (n, key)] = np.stack([ctx.fit_result(q, b.W) for q in range(n)])
np.savez(out, **res)
print("EARLY_BARRIER_CHILD_OK")
"""


def _child(out, early, nq):
    env = {k: v for k, v in os.environ.items() if k not in ("KP_GRAM3_COVER", "KP_GRAM3_ONEA", "KP_GRAM3_POW3", "KP_GRAM3_WGPCU", "KP_GRAM3_NQ",
                                                             "KP_GRAM3_LIFT_ORDER", "KP_GRAM_GROUP", "KP_GRAM3_EARLY_BARRIER")}
    if early is not None:
        env["KP_GRAM3_EARLY_BARRIER"] = str(early)
    if nq is not None:
        env["KP_GRAM3_NQ"] = str(nq)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out, str(nq)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "EARLY_BARRIER_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("early_barrier")
    cache = {}

    def get(nq):
        if nq not in cache:
            cache[nq] = {"new": _child(str(d / ("new_%s.npz" % nq)), None, nq), "old": _child(str(d / ("old_%s.npz" % nq)), 0, nq)}
        return cache[nq]
    return get


@pytest.fixture(scope="module")
def oracle():
    """Dense G = Px' Px, C = Px' Py of the oracle per dictionary at Ns = 4099; computed once, read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            nz, m, exps = DICTS[name][:3]
            Psi = lambda z: np.hstack([z, np.prod(z[:, None, :] ** exps()[None, :, :].astype(float), axis=2), np.ones((len(z), 1))])
            p = synth_pairs(4099, nz, m, seed=SEED)
            ut = np.hstack([np.ones((4099, 1)), p["u"]])
            Px = np.hstack([Psi(p["alpha"]) * ut[:, [a]] for a in range(m + 1)])
            Py = np.hstack([Psi(p["beta"]) * ut[:, [a]] for a in range(m + 1)])
            if name in ("headline", "head_m2", "poly2_m1"):          # full polynomial dictionaries: the oracle's own lift
                deg = 3 if name != "poly2_m1" else 2
                Pxo, Pyo = ko.px_py(ko.build_dictionary("bilinear", nz, m, ["poly"], [deg]), p)
                assert np.array_equal(Pxo.shape, Px.shape) and np.abs(Pxo - Px).max() <= 1e-13 * np.abs(Pxo).max()
                Px, Py = Pxo, Pyo
            Gr, Cr = Px.T @ Px, Px.T @ Py
            Gr.setflags(write=False); Cr.setflags(write=False)
            cache[name] = (Gr, Cr)
        return cache[name]
    return get


@pytest.mark.parametrize("Ns", NSS)
@pytest.mark.parametrize("nq,name", CASES)
def test_gram_bits_do_not_depend_on_the_barrier_placement(runs, oracle, nq, name, Ns):
    new, old = runs(nq)["new"], runs(nq)["old"]
    key = "%s_%d" % (name, Ns)
    G, C = new["G_" + key], new["C_" + key]
    tn, to = new["t_" + key], old["t_" + key]
    print(f"{name} NQ {nq} Ns {Ns}: timers 10 / 16 / 20 / 26 / 15 new {tn} old {to}; max|G| {np.abs(G).max():.3e} max|C| {np.abs(C).max():.3e}")
    assert np.isfinite(G).all() and np.isfinite(C).all() and np.abs(G).max() > 0
    assert np.array_equal(G, old["G_" + key]) and np.array_equal(C, old["C_" + key])
    assert tn[3] == _early_expected(name, nq, tn) and to[3] == 0.0   # early where the tile has the room, today's elsewhere and with the switch
    if name != "headline" or nq is not None:
        assert tn[3] == float(DICTS[name][5][nq])                # (the headline's circulant plan at NQ = 6 has jobs of two A groups)
    assert np.array_equal(tn[[0, 1, 2, 4]], to[[0, 1, 2, 4]])    # the same plan, table form and lift order in both
    assert tn[2] == (0.0 if name == "xyz80" else 1.0)
    if Ns == 4099:
        Gr, Cr = oracle(name)
        scale = np.abs(Gr).max()
        eg, ec = np.abs(G - Gr).max(), np.abs(C - Cr).max()
        print(f"  |G - Gr| {eg:.3e} |C - Cr| {ec:.3e} tol {1e-12 * scale:.3e}")
        assert G.shape == Gr.shape and eg <= 1e-12 * scale and ec <= 1e-12 * scale


@pytest.mark.parametrize("nq,name,Ns", [(nq, name, Ns) for nq, name in CASES for Ns in NSS if DICTS[name][3] < Ns])
def test_queues_of_pipelined_fits(runs, nq, name, Ns):
    new, old = runs(nq)["new"], runs(nq)["old"]
    key = "%s_%d" % (name, Ns)
    grp, W = int(new["group"]), DICTS[name][3]
    assert 1 <= grp <= 8 and grp == int(old["group"])
    for n in sorted({1, grp, grp + 1}):
        K, tq = new["Kq%d_%s" % (n, key)], new["tq%d_%s" % (n, key)]
        tqo = old["tq%d_%s" % (n, key)]
        print(f"{name} NQ {nq} Ns {Ns} queue of {n}: timers 10 / 16 / 20 / 26 / 15 new {tq} old {tqo}")
        assert K.shape == (n, W, W) and np.isfinite(K).all()
        assert np.array_equal(K, old["Kq%d_%s" % (n, key)]), (n, "bits of K differ between the barrier placements")
        assert tq[3] == float(DICTS[name][5][nq]) == _early_expected(name, nq, tq) and tqo[3] == 0.0
        assert np.array_equal(tq[[0, 1, 2, 4]], tqo[[0, 1, 2, 4]])
        if name == "headline" and nq is None:
            assert tq[0] == 184320.0                             # the one-A-group plan, as before
