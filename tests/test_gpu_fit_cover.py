"""GPU tests of the Kronecker Gram kernel's COVER plan (csrc/kp_gram3_cover.h, kp_gram3.hip): psi_x psi_x' of a monomial
dictionary from a subset of its 4 x 4 blocks that still forms every distinct monomial once, each entry of G written by the
reduction from its monomial's one designated source element.

KP_GRAM3_COVER is read once, hence fresh interpreters: `2` puts every launch of a qualifying dictionary on its cover plan,
kra.fit_gram included, `0` none.  The children compute, this process compares.

Shapes: Ns = 5 (one partial tile), 61 (8 tiles: fewer than splits), 4099 (513 tiles, the last one partial).
Dictionaries (states, inputs, degree, columns):
  headline   6, 3, 3       N = 84, W = 336                         cover KEPT: 143 quads -> 24 jobs of 6 (circulant 168 -> 28)
  w200       6, 3, 3, 50   its first 49 rows + the constant: padding columns in the last group   not kept (16 jobs either way)
  m2, m1     3, 2 | 1, 2   N = 10                                  not kept
  deg4       2, 1, 4       N = 15, fourth powers                   not kept
A cover plan is kept only when it has fewer whole workgroups than the circulant one, so the small dictionaries stay on the
circulant plan: with KP_GRAM3_COVER=2 they must report the circulant flop count (timer 10 equal to the `0` child's).  To put
the padding columns, fourth powers, m = 2 (three weight tuples) and m = 1 (unpaired weights) through a KEPT cover plan, four more:
  head_m2    6, 2, 3       N = 84       head_m1   6, 1, 3   N = 84
  n78        6, 3, 3, 78   N = 78: two padding columns
  p4s4       4, 3, 4       without x1 x2 x3 x4 (a column of the Kronecker kernel has at most three factors): N = 69, fourth powers,
                           three padding columns, 4 quads per job
(tools/gram3_cover_check.cpp prints these plans - p4s4 is `4 3 4 0 3`; tests/test_gram3_cover_plan.py checks them without a device.)

Tolerances: G, C against the oracle's dense products to 1e-12 max|G| (tests/test_gpu_fit.py); K of a pipelined fit against
the synchronous fit of the same object to 1e-11 max|K| (tests/test_gpu_fit.py, tests/test_gpu_fit_grouped.py).  Replacing
psi_i psi_j by another factorisation of the same monomial moves G by <= 1.2e-16 max|G| and K by <= 6e-15 max|K| on this
generator (numpy emulation, Ns = 4099 and 1e5: DESIGN 3.1).

C of the cover plan is bitwise the circulant plan's C WHERE BOTH SPLIT THE SNAPSHOTS ALIKE: a T block is the same MFMA chain
in either plan, but a lone launch deals its tiles over slots / nsuper splits, and a kept cover plan has fewer workgroups per
split (headline: 512 / 6 = 85 against 512 / 7 = 73).  At Ns = 5 and 61 every tile is its own split in both; at Ns = 4099 the
default geometry gives 7 against 8 tiles per split, so the comparison there runs both children with KP_GRAM3_WGPCU=6 (1 536
slots on the 256 CUs: 256 / 219 / 192 splits for 6 / 7 / 8 workgroups per split - the kept plans have 6 or 7, their circulant
ones 7 or 8 - and ceil(513 / .) = 3 tiles per split, 171 splits, for all of them), where the bits must agree as well.
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
DICTS = {"headline": (6, 3, 3, None), "w200": (6, 3, 3, 50), "m2": (3, 2, 2, None), "m1": (3, 1, 2, None), "deg4": (2, 1, 4, None),
         "head_m2": (6, 2, 3, None), "head_m1": (6, 1, 3, None), "n78": (6, 3, 3, 78), "p4s4": (4, 3, 4, "three_factors")}
KEPT = ("headline", "head_m2", "head_m1", "n78", "p4s4")
SEED = 40
WGPCU_ALIKE = 6      # (module docstring: the split geometry in which both plans walk Ns = 4099 in 171 splits of 3 tiles)


def _select(name):
    """Rows of the full polynomial table (states first) that the dictionary keeps; its constant column follows them."""
    nz, m, deg, sel = DICTS[name]
    tab = kra.poly_exponent_table(nz, deg)
    if sel is None:
        return tab, np.arange(len(tab))
    keep = np.arange(sel - 1) if isinstance(sel, int) else np.flatnonzero((tab > 0).sum(axis=1) <= 3)
    return tab, keep


def _rows(name):
    """Exponent rows of the dictionary's columns behind the states, and of all its columns (states first, constant last)."""
    nz = DICTS[name][0]
    tab, keep = _select(name)
    tab = tab[keep]
    return tab[nz:], np.vstack([tab, np.zeros((1, nz), np.uint8)]).astype(int)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from conftest import synth_pairs
from test_gpu_fit_cover import DICTS, SEED, _rows
out, names, nss, keep_g = sys.argv[2], sys.argv[3].split(","), [int(x) for x in sys.argv[4].split(",")], sys.argv[5] == "1"
ctx = kra.Context(0)
res = {}
for name in names:
    nz, m, deg, _ = DICTS[name]
    b = kra.Basis(ctx, "bilinear", nz, m, [("poly", _rows(name)[0])])
    for Ns in nss:
        p = synth_pairs(Ns, nz, m, seed=SEED)
        s = kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"])
        G, C = kra.fit_gram(ctx, b, s)
        res["t10_%s_%d" % (name, Ns)] = np.float64(ctx.timer(10))
        G2, C2 = kra.fit_gram(ctx, b, s)
        res["same_%s_%d" % (name, Ns)] = np.bool_(np.array_equal(G, G2) and np.array_equal(C, C2))
        res["C_%s_%d" % (name, Ns)] = C
        if keep_g:
            res["G_%s_%d" % (name, Ns)] = G
np.savez(out, **res)
print("COVER_CHILD_OK")
"""


def _child(out, cover, names, nss, keep_g, wgpcu=None):
    env = {k: v for k, v in os.environ.items() if k not in ("KP_GRAM3_COVER", "KP_GRAM3_WGPCU")}
    env["KP_GRAM3_COVER"] = str(cover)
    if wgpcu is not None:
        env["KP_GRAM3_WGPCU"] = str(wgpcu)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out, ",".join(names), ",".join(str(n) for n in nss), "1" if keep_g else "0"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "COVER_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cover")
    return {"cover": _child(str(d / "cover.npz"), 2, list(DICTS), NSS, True),
            "circ": _child(str(d / "circ.npz"), 0, list(DICTS), NSS, False),
            "cover_alike": _child(str(d / "cover_alike.npz"), 2, list(KEPT), (4099,), False, wgpcu=WGPCU_ALIKE),
            "circ_alike": _child(str(d / "circ_alike.npz"), 0, list(KEPT), (4099,), False, wgpcu=WGPCU_ALIKE)}


@pytest.fixture(scope="module")
def oracle():
    """Dense G = Px' Px, C = Px' Py of the oracle per (dictionary, Ns); computed once, read-only."""
    cache = {}

    def get(name, Ns):
        if (name, Ns) not in cache:
            nz, m, deg, sel = DICTS[name]
            dic = ko.build_dictionary("bilinear", nz, m, ["poly"], [deg])
            Px, Py = ko.px_py(dic, synth_pairs(Ns, nz, m, seed=SEED))
            if sel is not None:                    # the kept columns and the constant of every Kronecker block
                Nf = dic.N
                keep = np.concatenate([a * Nf + np.r_[_select(name)[1], Nf - 1] for a in range(m + 1)])
                Px, Py = Px[:, keep], Py[:, keep]
            Gr, Cr = Px.T @ Px, Px.T @ Py
            Gr.setflags(write=False); Cr.setflags(write=False)
            cache[(name, Ns)] = (Gr, Cr)
        return cache[(name, Ns)]
    return get


@pytest.mark.parametrize("Ns", NSS)
@pytest.mark.parametrize("name", list(DICTS))
def test_gram_of_every_launch_on_the_cover_plan(runs, oracle, name, Ns):
    r = runs["cover"]
    G, C = r["G_%s_%d" % (name, Ns)], r["C_%s_%d" % (name, Ns)]
    Gr, Cr = oracle(name, Ns)
    scale = np.abs(Gr).max()
    eg, ec = np.abs(G - Gr).max(), np.abs(C - Cr).max()
    print(f"{name} Ns {Ns}: |G - Gr| {eg:.3e} |C - Cr| {ec:.3e} tol {1e-12 * scale:.3e} timer10 {float(r['t10_%s_%d' % (name, Ns)]):.0f}")
    assert G.shape == Gr.shape and eg <= 1e-12 * scale and ec <= 1e-12 * scale
    assert np.array_equal(G, G.T)
    assert bool(r["same_%s_%d" % (name, Ns)])                       # two calls: the same bits
    t_cov, t_circ = float(r["t10_%s_%d" % (name, Ns)]), float(runs["circ"]["t10_%s_%d" % (name, Ns)])
    if name in KEPT:
        assert t_cov < t_circ, (t_cov, t_circ)
        # all entries of one (monomial, weight pair) come from one source element
        _, E = _rows(name)
        N, m = len(E), DICTS[name][1]
        key = (E[:, None, :] + E[None, :, :]).reshape(N * N, -1)
        _, idx, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        for a in range(m + 1):
            for b in range(m + 1):
                blk = G[a * N:(a + 1) * N, b * N:(b + 1) * N].reshape(-1)
                assert np.array_equal(blk, blk[idx][inv]), (name, Ns, a, b)
    else:
        assert t_cov == t_circ, (t_cov, t_circ)                    # no cover plan kept: the circulant plan ran
    if name == "headline":
        assert t_cov == 24 * 6 * 10 * 128 == 184320 and t_circ == 215040.0
    # C: the circulant plan's bits wherever the two plans split the snapshots alike (module docstring)
    if name not in KEPT or Ns < 4099:
        assert np.array_equal(C, runs["circ"]["C_%s_%d" % (name, Ns)])
    else:
        assert np.array_equal(runs["cover_alike"]["C_%s_%d" % (name, Ns)], runs["circ_alike"]["C_%s_%d" % (name, Ns)])
        assert float(runs["cover_alike"]["t10_%s_%d" % (name, Ns)]) == t_cov


def _basis(ctx, name):
    nz, m, _, _ = DICTS[name]
    return kra.Basis(ctx, "bilinear", nz, m, [("poly", _rows(name)[0])])


@pytest.mark.parametrize("name", ["headline", "n78", "head_m1"])
def test_default_mode_queue_takes_the_cover_plan_and_fit_gram_does_not(ctx, name):
    """Unset, the queue of the pipelined fits runs the cover plan and every other caller the circulant one: queues of 1, 2, G,
    G + 1 and 2 G + 3 fits return each object's own K within 1e-11 max|K| of its synchronous fit (circulant plan)."""
    G = int(ctx.timer(12))
    assert 1 <= G <= 8
    nz, m, _, _ = DICTS[name]
    b = _basis(ctx, name)
    W = b.W
    NWT = (m + 1) * (m + 2) // 2
    pairs = [synth_pairs(4099, nz, m, seed=300 + i) for i in range(2 * G + 3)]
    snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in pairs]
    Kref = [kra.fit(ctx, b, s)[0] for s in snaps]
    kra.fit_gram(ctx, b, snaps[0])
    t_circ = ctx.timer(10)
    for n in (1, 2, G, G + 1, 2 * G + 3):
        for i in range(n):
            kra.fit(ctx, b, snaps[i], fetch=False)
        ctx.synchronize()
        t_queue = ctx.timer(10)
        for q in range(n):
            err, tol = np.abs(ctx.fit_result(q, W) - Kref[q]).max(), 1e-11 * np.abs(Kref[q]).max()
            print(f"{name}: queue of {n}, result {q}: err {err:.3e} tol {tol:.3e}")
            assert err <= tol, (n, q)
        assert t_queue < t_circ, (t_queue, t_circ)
    if name == "headline":
        assert t_circ == 215040.0 and t_queue == 184320.0
    kra.fit_gram(ctx, b, snaps[0])
    assert ctx.timer(10) == t_circ
    assert t_circ % (NWT * 128) == 0
