"""GPU tests of the Kronecker Gram kernel's ordered lift (kp_gram3.hip: the LO form of the in-kernel-lift monomial kernel;
csrc/kp_gram3_lift.h).  The lift's (item, snapshot pair) jobs sit in the slots of a table built on the host: every job of three
real factors in lift step 0, real factors first, so that steps 1 and 2 read two table entries and multiply once.  A dropped
factor is exactly 1.0 and three-factor products keep their order, so G, C and K must be the SAME BITS as with
KP_GRAM3_LIFT_ORDER=0, which keeps the order e = tid + 256 j for every dictionary.

KP_GRAM3_LIFT_ORDER is read once, hence fresh interpreters: one child with the default, one with KP_GRAM3_LIFT_ORDER=0.  Neither
sets another switch: kra.fit_gram runs the circulant plan (a lone launch), the queues of pipelined fits the dictionary's cover /
one-A-group plan in lone and grouped launches - every launch form of the kernel.  The children compute, this process compares.

Dictionaries (all bilinear); kp_timer_get(20) = 1 where the last Gram launch ran the slot table, 0 where it ran the old order:
  headline   6 states, 3 inputs, poly-3: N = 84, W = 336 (160 / 384 / 164 jobs of three / two / fewer real factors)        1
  head_m2    the same columns, 2 inputs                                                                                    1
  poly2_m1   3 states, 1 input, poly-2: N = 10, W = 20 (unpaired weights; no job of three factors)                         1
  poly4      4 states, 3 inputs, poly-4 without the one column of four variables: N = 69, W = 276 (fourth powers: the
             four-entry table)                                                                                             1
  xyz80      6 states, 3 inputs: the states, the 80 monomials of degree 3 and 4 in exactly three variables, the constant:
             N = 87, W = 348; 640 jobs of three real factors do not fit lift step 0: the old order                         0
Shapes: Ns = 5 (one partial tile), 61 (8 tiles: fewer than splits), 4099 (513 tiles, the last one partial, several per split).

Tolerances: bitwise equality between the children (np.array_equal).  Against the oracle's dense products at Ns = 4099: 1e-12
max|G| (tests/test_gpu_fit_cover.py).  K is only defined while the Gram matrix is positive definite, W < Ns: queues of 1, G and
G + 1 pipelined fits (G = kp_timer_get(12)) at Ns = 4099, poly2_m1 (W = 20) also at Ns = 61.
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
NSS = (5, 61, 4099)
SEED = 97


def _at_most_three_variables(nz, deg):
    t = kra.poly_exponent_table(nz, deg)[nz:]
    return t[(t > 0).sum(axis=1) <= 3]


def _exactly_three_variables(nz, deg):
    t = kra.poly_exponent_table(nz, deg)[nz:]
    return t[(t > 0).sum(axis=1) == 3]


# name: (states, inputs, exponent rows of the poly block, kp_timer_get(20) expected by default, W)
DICTS = {
    "headline": (6, 3, lambda: kra.poly_exponent_table(6, 3)[6:], 1, 336),
    "head_m2": (6, 2, lambda: kra.poly_exponent_table(6, 3)[6:], 1, 252),
    "poly2_m1": (3, 1, lambda: kra.poly_exponent_table(3, 2)[3:], 1, 20),
    "poly4": (4, 3, lambda: _at_most_three_variables(4, 4), 1, 276),
    "xyz80": (6, 3, lambda: _exactly_three_variables(6, 4), 0, 348),
}
QUEUED = [(name, Ns) for name in DICTS for Ns in NSS if DICTS[name][4] < Ns]

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from conftest import synth_pairs
from test_gpu_fit_lift_order import DICTS, NSS, SEED
out = sys.argv[2]
ctx = kra.Context(0)
grp = int(ctx.timer(12))
res = {"group": np.int64(grp)}
for name, (nz, m, exps, _, W) in DICTS.items():
    b = kra.Basis(ctx, "bilinear", nz, m, [("poly", exps())])
    assert b.W == W, (name, b.W)
    for Ns in NSS:
        key = "%s_%d" % (name, Ns)
        pairs = [synth_pairs(Ns, nz, m, seed=SEED + i) for i in range(grp + 1)]
        snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in pairs]
        G, C = kra.fit_gram(ctx, b, snaps[0])
        res["G_" + key], res["C_" + key] = G, C
        res["t_" + key] = np.array([ctx.timer(10), ctx.timer(16), ctx.timer(20)])
        if not W < Ns:
            continue
        for n in sorted({1, grp, grp + 1}):
            for i in range(n):
                kra.fit(ctx, b, snaps[i], fetch=False)
            ctx.synchronize()
            res["tq%d_%s" % (n, key)] = np.array([ctx.timer(10), ctx.timer(16), ctx.timer(20)])
            res["Kq%d_%s" % (n, key)] = np.stack([ctx.fit_result(q, b.W) for q in range(n)])
np.savez(out, **res)
print("LIFT_ORDER_CHILD_OK")
"""


def _child(out, lift_order):
    env = {k: v for k, v in os.environ.items() if k not in ("KP_GRAM3_COVER", "KP_GRAM3_ONEA", "KP_GRAM3_POW3", "KP_GRAM3_WGPCU", "KP_GRAM3_NQ",
                                                             "KP_GRAM3_LIFT_ORDER", "KP_GRAM_GROUP")}
    if lift_order is not None:
        env["KP_GRAM3_LIFT_ORDER"] = str(lift_order)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "LIFT_ORDER_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lift_order")
    return {"new": _child(str(d / "new.npz"), None), "old": _child(str(d / "old.npz"), 0)}


@pytest.fixture(scope="module")
def oracle():
    """Dense G = Px' Px, C = Px' Py of the oracle per dictionary at Ns = 4099; computed once, read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            nz, m, exps, _, _ = DICTS[name]
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
@pytest.mark.parametrize("name", list(DICTS))
def test_gram_bits_do_not_depend_on_the_lift_order(runs, oracle, name, Ns):
    new, old = runs["new"], runs["old"]
    key = "%s_%d" % (name, Ns)
    G, C = new["G_" + key], new["C_" + key]
    tn, to = new["t_" + key], old["t_" + key]
    print(f"{name} Ns {Ns}: timers 10 / 16 / 20 new {tn} old {to}; max|G| {np.abs(G).max():.3e} max|C| {np.abs(C).max():.3e}")
    assert np.isfinite(G).all() and np.isfinite(C).all() and np.abs(G).max() > 0
    assert np.array_equal(G, old["G_" + key]) and np.array_equal(C, old["C_" + key])
    assert tn[2] == float(DICTS[name][3]) and to[2] == 0.0       # "ordered" where expected, "old" for the fall-back and with the switch
    assert tn[0] == to[0] and tn[1] == to[1]                     # the same plan and table form in both
    assert tn[1] == (4.0 if name == "poly4" else 3.0)
    if Ns == 4099:
        Gr, Cr = oracle(name)
        scale = np.abs(Gr).max()
        eg, ec = np.abs(G - Gr).max(), np.abs(C - Cr).max()
        print(f"  |G - Gr| {eg:.3e} |C - Cr| {ec:.3e} tol {1e-12 * scale:.3e}")
        assert G.shape == Gr.shape and eg <= 1e-12 * scale and ec <= 1e-12 * scale


@pytest.mark.parametrize("name,Ns", QUEUED)
def test_queues_of_pipelined_fits(runs, name, Ns):
    new, old = runs["new"], runs["old"]
    key = "%s_%d" % (name, Ns)
    grp, W = int(new["group"]), DICTS[name][4]
    assert 1 <= grp <= 8 and grp == int(old["group"])
    for n in sorted({1, grp, grp + 1}):
        K, tq = new["Kq%d_%s" % (n, key)], new["tq%d_%s" % (n, key)]
        assert K.shape == (n, W, W) and np.isfinite(K).all()
        assert np.array_equal(K, old["Kq%d_%s" % (n, key)]), (n, "bits of K differ between the lift orders")
        assert tq[2] == float(DICTS[name][3]) and old["tq%d_%s" % (n, key)][2] == 0.0
        assert tq[0] == old["tq%d_%s" % (n, key)][0]
        if name == "headline":
            assert tq[0] == 184320.0                             # the one-A-group plan, as before
