"""GPU tests of the two forms of the batched solve of pipelined fits (kp_solve.hip: kp_chol_solve_batch_dev, nb > 1).

KP_SOLVE_BATCH_FORM unset (or 1): systems up to n = 384 are substituted by kp_trsm2_batch_kernel - six row blocks per wave and
two workgroups per CU, a flat grid in kp_solve_xcd_map order (a system's column blocks on one die), C read from the [G | C] ring
and K stored into its slot of the result ring, no padded copy of C and no unpad launch.  KP_SOLVE_BATCH_FORM=0: pad G and C,
kp_trsm2_kernel<4> on a (column block, system) grid, unpad - the sequence of before.  Both run the same MFMA chains in the same
order: K must be the SAME BITS.  The switch is read once, hence fresh interpreters (as tests/test_gpu_fit_pow3.py): the
children compute, this process compares.

kp_timer_get(18) = 100 E + 10 X + C of the most recent batched solve: 211 the new entry, 100 the old one.

Dictionaries (all bilinear, W = N (m + 1)); Ns = 4 W, so that G is positive definite:
  w16    2 states, 1 input,  5 monomials:  N = 8,   W = 16    one row block, waves 1-3 own nothing
  w40    2 states, 3 inputs, poly-3:       N = 10,  W = 40    n = 48: padding predicates on the load of C and the store of K
  w336   6 states, 3 inputs, poly-3:       N = 84,  W = 336   21 blocks: waves own 6, 5, 5, 5
  w384   6 states, 3 inputs, 89 monomials: N = 96,  W = 384   the new entry's limit, every wave owns 6
  w400   6 states, 3 inputs, 93 monomials: N = 100, W = 400   beyond it: the old entry in both children (E = 1)
Queues of 2, 9 and 17 pipelined fits (not multiples of 8; more systems than dies), one batched solve each.

Per dictionary G, C of kra.fit_gram of each snapshot object; K of a queue against numpy.linalg.solve(G, C) within 1e-11 max|K|,
the bound tests/test_gpu_fit_grouped.py holds pipelined fits to against synchronous ones.

wrap: w40 with a result ring of 5 slots: 3 fits, a refill that grows another snapshot object (it launches the queued solves
without closing the batch), 5 more fits - the second batch starts at slot 3 and wraps inside the batch.
notspd: w40, a queue of 9 whose member 4 has a duplicated state column - its Gram matrix is singular, the factorisation stops,
kp_synchronize reports it; its K slot holds its C, the other slots their K, in both forms alike.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_realizations_amd as kra

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 211
BATCHES = (2, 9, 17)
WRAP_SLOTS, WRAP_FIRST, WRAP_SECOND = 5, 3, 5
BAD_BATCH, BAD_MEMBER = 9, 4

# name: (states, inputs, exponent rows of the poly block, W, code of timer 18 in the new form)
DICTS = {
    "w16": (2, 1, lambda: kra.poly_exponent_table(2, 3)[2:][:5], 16, 211.0),
    "w40": (2, 3, lambda: kra.poly_exponent_table(2, 3)[2:], 40, 211.0),
    "w336": (6, 3, lambda: kra.poly_exponent_table(6, 3)[6:], 336, 211.0),
    "w384": (6, 3, lambda: kra.poly_exponent_table(6, 4)[6:][:89], 384, 211.0),
    "w400": (6, 3, lambda: kra.poly_exponent_table(6, 4)[6:][:93], 400, 100.0),
}

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from conftest import synth_pairs
from test_gpu_solve_batch_forms import DICTS, BATCHES, SEED, WRAP_SLOTS, WRAP_FIRST, WRAP_SECOND, BAD_BATCH, BAD_MEMBER
out = sys.argv[2]
ctx = kra.Context(0)
res = {}
nmax = max(BATCHES)
for name, (nz, m, exps, W, _) in DICTS.items():
    b = kra.Basis(ctx, "bilinear", nz, m, [("poly", exps())])
    assert b.W == W, (name, b.W)
    Ns = 4 * W
    pairs = [synth_pairs(Ns, nz, m, seed=SEED + i) for i in range(nmax)]
    snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in pairs]
    GC = [kra.fit_gram(ctx, b, s) for s in snaps]
    res["G_" + name] = np.stack([g for g, _ in GC]); res["C_" + name] = np.stack([c for _, c in GC])
    for nb in BATCHES:
        for i in range(nb):
            kra.fit(ctx, b, snaps[i], fetch=False)
        ctx.synchronize()
        res["t_%s_%d" % (name, nb)] = np.float64(ctx.timer(18))
        res["K_%s_%d" % (name, nb)] = np.stack([ctx.fit_result(q, W) for q in range(nb)])
    if name != "w40":
        continue
    # the ring wraps inside a batch that does not start at slot 0
    ctx.fit_async_slots(WRAP_SLOTS)
    small = synth_pairs(8, nz, m, seed=SEED + 100)
    other = kra.Snapshots(ctx, small["alpha"], small["beta"], small["u"])
    for i in range(WRAP_FIRST):
        kra.fit(ctx, b, snaps[i], fetch=False)
    grown = synth_pairs(64, nz, m, seed=SEED + 101)
    other.update(grown["alpha"], grown["beta"], grown["u"])          # grows: the queued solves are launched, the batch stays open
    for i in range(WRAP_FIRST, WRAP_FIRST + WRAP_SECOND):
        kra.fit(ctx, b, snaps[i], fetch=False)
    ctx.synchronize()
    res["t_wrap"] = np.float64(ctx.timer(18))
    res["K_wrap"] = np.stack([ctx.fit_result(q, W) for q in range(WRAP_FIRST, WRAP_FIRST + WRAP_SECOND)])
    ctx.fit_async_slots(128)
    # a Gram matrix that is not positive definite in the middle of a batch
    p = dict(pairs[BAD_MEMBER])
    p["alpha"] = p["alpha"].copy(); p["alpha"][:, 1] = p["alpha"][:, 0]
    bad = kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"])
    Gb, Cb = kra.fit_gram(ctx, b, bad)
    res["G_bad"], res["C_bad"] = Gb, Cb
    for i in range(BAD_BATCH):
        kra.fit(ctx, b, bad if i == BAD_MEMBER else snaps[i], fetch=False)
    err = ""
    try:
        ctx.synchronize()
    except kra.KoopmanHipError as e:
        err = str(e)
    res["err_bad"] = np.array(err)
    res["t_bad"] = np.float64(ctx.timer(18))
    res["K_bad"] = np.stack([ctx.fit_result(q, W) for q in range(BAD_BATCH)])
np.savez(out, **res)
print("SOLVE_FORMS_CHILD_OK")
"""


def _child(out, form):
    env = {k: v for k, v in os.environ.items() if k not in ("KP_SOLVE_BATCH_FORM", "KP_SOLVE_BATCH", "KP_NO_ASYNC", "KP_GRAM_GROUP")}
    if form is not None:
        env["KP_SOLVE_BATCH_FORM"] = str(form)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SOLVE_FORMS_CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("solve_forms")
    return {"new": _child(str(d / "new.npz"), None), "old": _child(str(d / "old.npz"), 0)}


@pytest.fixture(scope="module")
def kref(runs):
    """numpy.linalg.solve(G, C) per dictionary and snapshot object, computed once"""
    new = runs["new"]
    return {name: np.stack([np.linalg.solve(g, c) for g, c in zip(new["G_" + name], new["C_" + name])]) for name in DICTS}


@pytest.mark.parametrize("nb", BATCHES)
@pytest.mark.parametrize("name", list(DICTS))
def test_k_of_a_batch_is_the_same_bits_in_both_forms(runs, kref, name, nb):
    new, old = runs["new"], runs["old"]
    W, code = DICTS[name][3], DICTS[name][4]
    key = "%s_%d" % (name, nb)
    K = new["K_" + key]
    print(f"{name} batch {nb}: timer 18 new {float(new['t_' + key])} old {float(old['t_' + key])}")
    assert float(new["t_" + key]) == code and float(old["t_" + key]) == 100.0
    assert K.shape == (nb, W, W) and np.isfinite(K).all()
    assert np.array_equal(new["G_" + name], old["G_" + name]) and np.array_equal(new["C_" + name], old["C_" + name])
    assert np.array_equal(K, old["K_" + key]), "bits of K differ between the forms of the batched solve"
    for q in range(nb):
        err, tol = np.abs(K[q] - kref[name][q]).max(), 1e-11 * np.abs(kref[name][q]).max()
        print(f"{name} batch {nb}, result {q}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (nb, q)


def test_ring_that_wraps_inside_a_batch(runs, kref):
    new, old = runs["new"], runs["old"]
    K = new["K_wrap"]
    assert (WRAP_FIRST % WRAP_SLOTS) != 0 and WRAP_FIRST % WRAP_SLOTS + WRAP_SECOND > WRAP_SLOTS       # starts off slot 0 and wraps
    assert float(new["t_wrap"]) == 211.0 and float(old["t_wrap"]) == 100.0
    assert K.shape == (WRAP_SECOND, 40, 40)
    assert np.array_equal(K, old["K_wrap"])
    for i in range(WRAP_SECOND):
        ref = kref["w40"][WRAP_FIRST + i]
        err, tol = np.abs(K[i] - ref).max(), 1e-11 * np.abs(ref).max()
        print(f"wrap: fit {WRAP_FIRST + i}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, i


def test_a_gram_matrix_that_is_not_positive_definite_in_the_middle_of_a_batch(runs, kref):
    new, old = runs["new"], runs["old"]
    K = new["K_bad"]
    print("error:", str(new["err_bad"]))
    assert "not numerically positive definite" in str(new["err_bad"]) and str(new["err_bad"]) == str(old["err_bad"])
    assert float(new["t_bad"]) == 211.0 and float(old["t_bad"]) == 100.0
    assert np.array_equal(new["G_bad"], old["G_bad"]) and np.array_equal(new["C_bad"], old["C_bad"])
    assert np.array_equal(K, old["K_bad"])
    assert np.array_equal(K[BAD_MEMBER], new["C_bad"])                       # the failed system's slot: its C, copied through
    for q in range(BAD_BATCH):
        if q == BAD_MEMBER:
            continue
        err, tol = np.abs(K[q] - kref["w40"][q]).max(), 1e-11 * np.abs(kref["w40"][q]).max()
        print(f"notspd: result {q}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol, q
