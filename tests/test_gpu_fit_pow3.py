"""GPU tests of the Kronecker Gram kernel's three-entry power table (kp_gram3.hip: the P3 form of the in-kernel-lift monomial
kernel).  The in-loop table build writes x, x^2, x^3, x^4 per raw value; a dictionary without fourth powers never reads the x^4
entry, so its launches run a form that neither computes nor stores it.  That removes a value nothing reads: G and C must be the
SAME BITS as with KP_GRAM3_POW3=0, which keeps four entries for every dictionary, and a dictionary WITH fourth powers must stay on
four entries.

KP_GRAM3_POW3 and KP_GRAM3_COVER are read once, hence fresh interpreters: both children run with KP_GRAM3_COVER=2, which puts
kra.fit_gram on the plan of the pipelined launches, one child with KP_GRAM3_POW3=0.  The children compute, this process compares.

Dictionaries (all bilinear); kp_timer_get(16) = table entries written per raw value by the last Gram launch:
  headline   6 states, 3 inputs, poly-3: N = 84, W = 336 (five weight tuples)                              3
  head_m2    the same columns, 2 inputs (three weight tuples)                                              3
  head_m1    the same columns, 1 input (unpaired weights)                                                  3
  xyz32      6 states, 3 inputs: the states, 32 monomials of three distinct variables out of the first
             four states (x y z, x^2 y z, x^2 y^2 z, x^3 y z), the constant: N = 39, a custom exponent list  3
  deg4       2 states, 1 input, poly-4 (N = 15; tests/test_gpu_fit_cover.py's fourth-power shape)          4
Shapes: Ns = 5 (one partial tile), 61 (8 tiles: fewer than splits), 4099 (513 tiles, the last one partial, several per split).

Per (dictionary, Ns) each child stores G, C of kra.fit_gram and kp_timer_get(10 / 15 / 16) behind it: G and C are bitwise equal
between the two children and timer 16 reports the form.  K is only defined while the Gram matrix is positive definite, W < Ns
(tests/test_gpu_fit_grouped.py): every dictionary at Ns = 4099, deg4 (W = 30) also at Ns = 61 (fewer tiles than splits in a
group launch).  There each child also runs queues of 1 and of G = kp_timer_get(12) pipelined fits and the synchronous fit of the
same snapshot objects: K of a queue is within 1e-11 max|K| of the synchronous K (that file's tolerance) and bitwise equal
between the two children.
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_realizations_amd as kra

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSS = (5, 61, 4099)
SEED = 83


def three_variable_monomials(count, nz=6):
    """`count` exponent rows of three distinct variables out of the first four of nz states, powers <= 3, in a fixed order:
    x y z (4), x^2 y z (12), x^2 y^2 z (12), x^3 y z (12)."""
    rows = []
    for pows in ((1, 1, 1), (2, 1, 1), (2, 2, 1), (3, 1, 1)):
        for trip in itertools.combinations(range(4), 3):
            for perm in sorted(set(itertools.permutations(pows))):
                r = [0] * nz
                for v, e in zip(trip, perm):
                    r[v] = e
                rows.append(r)
    assert len(rows) == 40 and len({tuple(r) for r in rows}) == 40
    return np.array(rows[:count], np.uint8)


# name: (states, inputs, exponent rows of the poly block, table entries expected, W)
DICTS = {
    "headline": (6, 3, lambda: kra.poly_exponent_table(6, 3)[6:], 3, 336),
    "head_m2": (6, 2, lambda: kra.poly_exponent_table(6, 3)[6:], 3, 252),
    "head_m1": (6, 1, lambda: kra.poly_exponent_table(6, 3)[6:], 3, 168),
    "xyz32": (6, 3, lambda: three_variable_monomials(32), 3, 156),
    "deg4": (2, 1, lambda: kra.poly_exponent_table(2, 4)[2:], 4, 30),
}
QUEUED = [(name, Ns) for name in DICTS for Ns in NSS if DICTS[name][4] < Ns]

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from conftest import synth_pairs
from test_gpu_fit_pow3 import DICTS, NSS, SEED
out = sys.argv[2]
ctx = kra.Context(0)
grp = int(ctx.timer(12))
res = {"group": np.int64(grp)}
for name, (nz, m, exps, _, W) in DICTS.items():
    b = kra.Basis(ctx, "bilinear", nz, m, [("poly", exps())])
    assert b.W == W, (name, b.W)
    for Ns in NSS:
        key = "%s_%d" % (name, Ns)
        pairs = [synth_pairs(Ns, nz, m, seed=SEED + i) for i in range(grp)]
        snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in pairs]
        G, C = kra.fit_gram(ctx, b, snaps[0])
        res["G_" + key], res["C_" + key] = G, C
        res["t_" + key] = np.array([ctx.timer(10), ctx.timer(15), ctx.timer(16)])
        if not W < Ns:
            continue
        res["Kref_" + key] = np.stack([kra.fit(ctx, b, s)[0] for s in snaps])
        for n in sorted({1, grp}):
            for i in range(n):
                kra.fit(ctx, b, snaps[i], fetch=False)
            ctx.synchronize()
            res["tq%d_%s" % (n, key)] = np.array([ctx.timer(10), ctx.timer(15), ctx.timer(16)])
            res["Kq%d_%s" % (n, key)] = np.stack([ctx.fit_result(q, b.W) for q in range(n)])
np.savez(out, **res)
print("POW3_CHILD_OK")
"""


def _child(out, pow3):
    env = {k: v for k, v in os.environ.items() if k not in ("KP_GRAM3_COVER", "KP_GRAM3_ONEA", "KP_GRAM3_POW3", "KP_GRAM3_WGPCU", "KP_GRAM3_NQ")}
    env["KP_GRAM3_COVER"] = "2"
    if pow3 is not None:
        env["KP_GRAM3_POW3"] = str(pow3)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "POW3_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pow3")
    return {"new": _child(str(d / "new.npz"), None), "old": _child(str(d / "old.npz"), 0)}


@pytest.mark.parametrize("Ns", NSS)
@pytest.mark.parametrize("name", list(DICTS))
def test_gram_bits_do_not_depend_on_the_table_form(runs, name, Ns):
    new, old = runs["new"], runs["old"]
    key = "%s_%d" % (name, Ns)
    G, C = new["G_" + key], new["C_" + key]
    tn, to = new["t_" + key], old["t_" + key]
    print(f"{name} Ns {Ns}: timers 10 / 15 / 16 new {tn} old {to}; max|G| {np.abs(G).max():.3e} max|C| {np.abs(C).max():.3e}")
    assert np.isfinite(G).all() and np.isfinite(C).all() and np.abs(G).max() > 0
    assert np.array_equal(G, old["G_" + key]) and np.array_equal(C, old["C_" + key])
    assert tn[2] == float(DICTS[name][3]) and to[2] == 4.0
    assert tn[0] == to[0] and tn[1] == to[1]                     # the same plan in both
    if name == "headline":
        assert tn[0] == 184320.0 and tn[1] == 0.0


@pytest.mark.parametrize("name,Ns", QUEUED)
def test_queues_of_pipelined_fits(runs, name, Ns):
    new, old = runs["new"], runs["old"]
    key = "%s_%d" % (name, Ns)
    grp, W = int(new["group"]), DICTS[name][4]
    assert 1 <= grp <= 8 and grp == int(old["group"])
    Kref = new["Kref_" + key]
    for n in sorted({1, grp}):
        K, tq = new["Kq%d_%s" % (n, key)], new["tq%d_%s" % (n, key)]
        assert K.shape == (n, W, W)
        assert np.array_equal(K, old["Kq%d_%s" % (n, key)]), (n, "bits of K differ between the table forms")
        assert tq[2] == float(DICTS[name][3]) and old["tq%d_%s" % (n, key)][2] == 4.0
        if name == "headline":
            assert tq[0] == 184320.0 and tq[1] == 0.0
        for q in range(n):                                       # against the synchronous fit of the same object
            err, tol = np.abs(K[q] - Kref[q]).max(), 1e-11 * np.abs(Kref[q]).max()
            print(f"{name} Ns {Ns}: queue of {n}, result {q}: err {err:.3e} tol {tol:.3e}")
            assert err <= tol, (n, q)
