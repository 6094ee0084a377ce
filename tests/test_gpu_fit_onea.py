"""GPU tests of the Kronecker Gram kernel's ONE-A-GROUP cover plan (csrc/kp_gram3_cover.h: gram3_onea_build; kp_gram3.hip): the
cover plan's jobs and quads per job, but every job (wave) stays on one A group of psi_x - rows of the plan are whole jobs, a few hub
rows two - so a wave weighs one A fragment per k-step.  The kernel is the cover plan's, job headers a1 = a0, qs = nq.

KP_GRAM3_COVER and KP_GRAM3_ONEA are read once, hence fresh interpreters: KP_GRAM3_COVER=2 puts every launch of a qualifying
dictionary on its cover plan, kra.fit_gram included; KP_GRAM3_ONEA=0 keeps the cover plan of consecutive quads.  The children
compute, this process compares.

Dictionaries: the headline (6 states, 3 inputs, poly-3: N = 84, W = 336) and its m = 2 sibling (three weight tuples).
Shapes: Ns = 5 (one partial tile), 61 (8 tiles: fewer than splits), 4099 (513 tiles, the last one partial, several tiles per split).

Tolerances: G, C against the oracle's dense products to 1e-12 max|G| (tests/test_gpu_fit.py, tests/test_gpu_fit_cover.py); K of a
pipelined fit against the synchronous fit of the same object to 1e-11 max|K| (tests/test_gpu_fit_grouped.py).  G comes from other
factorisations of the same monomials than the cover plan's, the last bits move; C does not: a T block is the same MFMA chain in all
three plans.  The one-A-group plan and the cover plan have the same number of workgroups per split, hence the same splits at every
Ns; the circulant plan has one more, so its C is compared where every tile is its own split in both (Ns = 5 and 61).
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
DICTS = {"headline": (6, 3, 3), "head_m2": (6, 2, 3)}
SEED = 41

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from conftest import synth_pairs
from test_gpu_fit_onea import DICTS, SEED
out, nss, keep_g = sys.argv[2], [int(x) for x in sys.argv[3].split(",")], sys.argv[4] == "1"
ctx = kra.Context(0)
res = {}
for name, (nz, m, deg) in DICTS.items():
    b = kra.Basis(ctx, "bilinear", nz, m, [("poly", kra.poly_exponent_table(nz, deg)[nz:])])
    for Ns in nss:
        p = synth_pairs(Ns, nz, m, seed=SEED)
        s = kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"])
        G, C = kra.fit_gram(ctx, b, s)
        res["t10_%s_%d" % (name, Ns)] = np.float64(ctx.timer(10))
        res["t15_%s_%d" % (name, Ns)] = np.float64(ctx.timer(15))
        G2, C2 = kra.fit_gram(ctx, b, s)
        res["same_%s_%d" % (name, Ns)] = np.bool_(np.array_equal(G, G2) and np.array_equal(C, C2))
        res["C_%s_%d" % (name, Ns)] = C
        if keep_g:
            res["G_%s_%d" % (name, Ns)] = G
np.savez(out, **res)
print("ONEA_CHILD_OK")
"""


def _child(out, cover, onea, nss, keep_g):
    env = {k: v for k, v in os.environ.items() if k not in ("KP_GRAM3_COVER", "KP_GRAM3_ONEA", "KP_GRAM3_WGPCU", "KP_GRAM3_NQ")}
    env["KP_GRAM3_COVER"] = str(cover)
    if onea is not None:
        env["KP_GRAM3_ONEA"] = str(onea)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out, ",".join(str(n) for n in nss), "1" if keep_g else "0"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ONEA_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("onea")
    return {"onea": _child(str(d / "onea.npz"), 2, None, NSS, True),
            "cover": _child(str(d / "cover.npz"), 2, 0, NSS, False),
            "circ": _child(str(d / "circ.npz"), 0, None, (5, 61), False)}


@pytest.fixture(scope="module")
def oracle():
    """Dense G = Px' Px, C = Px' Py of the oracle per (dictionary, Ns); computed once, read-only."""
    cache = {}

    def get(name, Ns):
        if (name, Ns) not in cache:
            nz, m, deg = DICTS[name]
            dic = ko.build_dictionary("bilinear", nz, m, ["poly"], [deg])
            Px, Py = ko.px_py(dic, synth_pairs(Ns, nz, m, seed=SEED))
            Gr, Cr = Px.T @ Px, Px.T @ Py
            Gr.setflags(write=False); Cr.setflags(write=False)
            cache[(name, Ns)] = (Gr, Cr)
        return cache[(name, Ns)]
    return get


@pytest.mark.parametrize("Ns", NSS)
@pytest.mark.parametrize("name", list(DICTS))
def test_gram_of_every_launch_on_the_one_a_group_plan(runs, oracle, name, Ns):
    r, rc = runs["onea"], runs["cover"]
    key = "%s_%d" % (name, Ns)
    G, C = r["G_" + key], r["C_" + key]
    Gr, Cr = oracle(name, Ns)
    scale = np.abs(Gr).max()
    eg, ec = np.abs(G - Gr).max(), np.abs(C - Cr).max()
    t10, t15, t10c, t15c = float(r["t10_" + key]), float(r["t15_" + key]), float(rc["t10_" + key]), float(rc["t15_" + key])
    print(f"{name} Ns {Ns}: |G - Gr| {eg:.3e} |C - Cr| {ec:.3e} tol {1e-12 * scale:.3e} timer10 {t10:.0f} / {t10c:.0f} timer15 {t15:.0f} / {t15c:.0f}")
    assert G.shape == Gr.shape and eg <= 1e-12 * scale and ec <= 1e-12 * scale
    assert np.array_equal(G, G.T)
    assert bool(r["same_" + key]) and bool(rc["same_" + key])        # two calls: the same bits
    # all entries of one (monomial, weight pair) come from one source element
    nz, m, deg = DICTS[name]
    E = np.vstack([kra.poly_exponent_table(nz, deg), np.zeros((1, nz), np.uint8)]).astype(int)
    N = len(E)
    mono = (E[:, None, :] + E[None, :, :]).reshape(N * N, -1)
    _, idx, inv = np.unique(mono, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    for a in range(m + 1):
        for b in range(m + 1):
            blk = G[a * N:(a + 1) * N, b * N:(b + 1) * N].reshape(-1)
            assert np.array_equal(blk, blk[idx][inv]), (name, Ns, a, b)
    # no job spans two A groups with the plan on, some do with KP_GRAM3_ONEA=0; the work on the matrix pipe is the same
    assert t15 == 0.0 and t15c > 0.0
    assert t10 == t10c
    if name == "headline":
        assert t10 == 24 * 6 * 10 * 128 == 184320 and t15c == 17.0
    # C: the cover plan's bits at every count (same workgroups per split, same splits), the circulant plan's where every tile is a split
    assert np.array_equal(C, rc["C_" + key])
    if Ns < 4099:
        assert np.array_equal(C, runs["circ"]["C_" + key])


@pytest.mark.parametrize("name", list(DICTS))
def test_queue_of_pipelined_fits_takes_the_one_a_group_plan(ctx, name):
    """Unset, the queue of the pipelined fits runs the one-A-group plan and every other caller the circulant one: queues of 1, G and
    G + 1 fits return each object's own K within 1e-11 max|K| of its synchronous fit."""
    G = int(ctx.timer(12))
    assert 1 <= G <= 8
    nz, m, deg = DICTS[name]
    b = kra.Basis(ctx, "bilinear", nz, m, [("poly", kra.poly_exponent_table(nz, deg)[nz:])])
    W = b.W
    pairs = [synth_pairs(4099, nz, m, seed=400 + i) for i in range(G + 1)]
    snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in pairs]
    Kref = [kra.fit(ctx, b, s)[0] for s in snaps]
    kra.fit_gram(ctx, b, snaps[0])
    t10_circ, t15_circ = ctx.timer(10), ctx.timer(15)
    assert t15_circ > 0
    for n in (1, G, G + 1):
        for i in range(n):
            kra.fit(ctx, b, snaps[i], fetch=False)
        ctx.synchronize()
        t10, t15 = ctx.timer(10), ctx.timer(15)
        for q in range(n):
            err, tol = np.abs(ctx.fit_result(q, W) - Kref[q]).max(), 1e-11 * np.abs(Kref[q]).max()
            print(f"{name}: queue of {n}, result {q}: err {err:.3e} tol {tol:.3e}")
            assert err <= tol, (n, q)
        assert t15 == 0.0 and t10 < t10_circ, (t15, t10, t10_circ)
    if name == "headline":
        assert t10 == 184320.0
