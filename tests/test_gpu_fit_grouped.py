"""GPU tests of the pipelined fits' Gram queue: up to KP_GRAM_GROUP queued fits of one dictionary and snapshot count share ONE
Kronecker Gram launch and ONE split-partial reduction (kp_fit.hip: kp_flush_grams; kp_gram3.hip: the group launch).

Reference: the synchronous fit `kra.fit(ctx, b, s)[0]` of each snapshot object.  Tolerance: 1e-11 max|K_ref|, the one
tests/test_gpu_fit.py uses for pipelined against synchronous fits on this generator (a group member sums its snapshots over
another number of splits than a lone launch: the same terms in another, still fixed, order).

Dictionaries: the headline (bilinear poly-3 on 6 states, m = 3: W = 336, five weight tuples), and bilinear poly-2 on 3 states
with m = 2 (three tuples) and m = 1 (three unpaired weights); at Ns = 4099 also the part of the headline dictionary that is
linear in the states, [x, 1] (x) [1, u] on 6 states with m = 3 (W = 28: the headline's weights on a small plan).  Ns = 4099 is 513
tiles of 8 snapshots with a partial last one - more tiles than any fit has splits.  Ns = 61 (8 tiles) and Ns = 5 (1 tile) have fewer tiles than splits, so most splits
contribute exact zeros; K is only defined while the Gram matrix is positive definite, i.e. W < Ns: the poly-2 dictionaries
(W = 30, 20) serve Ns = 61, and Ns = 5 takes the smallest bilinear dictionary there is, [x, 1] (x) [1, u] on one state (W = 4).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from conftest import synth_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 4099
DICTS = {"headline": (6, 3, 3), "headline_lin": (6, 3, 1), "m2": (3, 2, 2), "m1": (3, 1, 2), "tiny": (1, 1, 1)}       # name -> (states, inputs, degree)


def _basis(ctx, name):
    nz, m, deg = DICTS[name]
    return kra.Basis(ctx, "bilinear", nz, m, [("poly", kra.poly_exponent_table(nz, deg)[nz:])])


def _tol(Kref):
    return 1e-11 * np.abs(Kref).max()


@pytest.fixture(scope="module")
def G(ctx):
    """The library's group size (KP_GRAM_GROUP or its default; read once per process)."""
    g = int(ctx.timer(12))
    assert 1 <= g <= 8
    return g


class _Set:
    """A dictionary, n snapshot objects of one count and the synchronous K of each (computed once, never changed)."""

    def __init__(self, ctx, name, n, Ns, seed0):
        nz, m, _ = DICTS[name]
        self.b = _basis(ctx, name)
        self.W = self.b.W
        self.pairs = [synth_pairs(Ns, nz, m, seed=seed0 + i) for i in range(n)]
        self.snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in self.pairs]
        self.Kref = [kra.fit(ctx, self.b, s)[0] for s in self.snaps]
        for K in self.Kref:
            K.setflags(write=False)


@pytest.fixture(scope="module")
def sets(ctx, G):
    return {name: _Set(ctx, name, 2 * G + 3, NS, 100 * (i + 1)) for i, name in enumerate(("headline", "m2", "m1", "headline_lin"))}


def _check_queue(ctx, st, idx, G):
    """Queues the objects idx in order, synchronises once, checks that the fits ran in groups of G (and a rest), compares every
    result with its own object's reference."""
    for i in idx:
        kra.fit(ctx, st.b, st.snaps[i], fetch=False)
    ctx.synchronize()
    # Launches of several fits are always timed, single ones every 4th time: timer 7 counts the timed launches, timer 13 the fits
    # they served.  len(idx) fits make len // G full groups and a rest; fits that did not group would give timer 13 == timer 7.
    n, launches, served = len(idx), int(ctx.timer(7)), int(ctx.timer(13))
    sizes = [G] * (n // G) + ([n % G] if n % G else [])
    multi = [z for z in sizes if z > 1]
    ones = len(sizes) - len(multi)
    print(f"queue of {n}: groups {sizes}, timed launches {launches}, fits served {served}")
    assert len(multi) <= launches <= len(multi) + max(ones, 0 if multi else 1), (sizes, launches)
    assert served - launches == sum(multi) - len(multi), (sizes, launches, served)
    for q, i in enumerate(idx):
        err = np.abs(ctx.fit_result(q, st.W) - st.Kref[i]).max()
        print(f"queue of {len(idx)}: result {q} (object {i}) err {err:.3e} tol {_tol(st.Kref[i]):.3e}")
        assert err <= _tol(st.Kref[i]), (len(idx), q, i)


@pytest.mark.parametrize("name", ["headline", "m2", "m1", "headline_lin"])
def test_every_group_size_returns_each_objects_own_fit_in_issue_order(ctx, G, sets, name):
    st = sets[name]
    for n in (1, 2, 3, G, G + 1, 2 * G + 3):
        _check_queue(ctx, st, list(range(n)), G)


@pytest.mark.parametrize("name,Ns", [("m2", 61), ("m1", 61), ("tiny", 5)])
def test_fewer_tiles_than_splits(ctx, G, name, Ns):
    st = _Set(ctx, name, max(G, 3), Ns, 700 + Ns)
    assert st.W < Ns
    _check_queue(ctx, st, list(range(G)), G)
    _check_queue(ctx, st, [0, 1, 2], G)


def test_same_object_twice_in_one_group_gives_bitwise_equal_results(ctx, G, sets):
    st = sets["headline"]
    kra.fit(ctx, st.b, st.snaps[0], fetch=False)
    kra.fit(ctx, st.b, st.snaps[0], fetch=False)
    ctx.synchronize()
    K0, K1 = ctx.fit_result(0, st.W), ctx.fit_result(1, st.W)
    assert np.array_equal(K0, K1)
    assert np.abs(K0 - st.Kref[0]).max() <= _tol(st.Kref[0])


def test_result_ring_smaller_than_the_group(ctx, G, sets):
    st = sets["m2"]
    ctx.fit_async_slots(2)
    try:
        for i in range(5):
            kra.fit(ctx, st.b, st.snaps[i], fetch=False)
        for q in (3, 4):
            assert np.abs(ctx.fit_result(q, st.W) - st.Kref[q]).max() <= _tol(st.Kref[q]), q
        for q in (0, 1, 2):
            with pytest.raises(kra.KoopmanHipError) as e:
                ctx.fit_result(q, st.W)
            assert e.value.code == F.KP_ERR_ARG
    finally:
        ctx.fit_async_slots(128)


def test_queue_is_launched_before_a_refill_and_before_a_close(ctx, G):
    nz, m, _ = DICTS["m2"]
    b = _basis(ctx, "m2")
    W = b.W
    pA, pB, pA2 = (synth_pairs(NS, nz, m, seed=s) for s in (801, 802, 803))
    ref = [kra.fit(ctx, b, kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]))[0] for p in (pA, pB, pA2)]
    A = kra.Snapshots(ctx, pA["alpha"], pA["beta"], pA["u"])
    B = kra.Snapshots(ctx, pB["alpha"], pB["beta"], pB["u"])
    kra.fit(ctx, b, A, fetch=False)
    kra.fit(ctx, b, B, fetch=False)
    A.update(pA2["alpha"], pA2["beta"], pA2["u"])
    kra.fit(ctx, b, A, fetch=False)
    ctx.synchronize()
    assert np.abs(ctx.fit_result(0, W) - ref[0]).max() <= _tol(ref[0])          # the OLD data's K
    assert np.abs(ctx.fit_result(1, W) - ref[1]).max() <= _tol(ref[1])
    assert np.abs(ctx.fit_result(2, W) - ref[2]).max() <= _tol(ref[2])          # the new data's
    A2 = kra.Snapshots(ctx, pA["alpha"], pA["beta"], pA["u"])
    kra.fit(ctx, b, A2, fetch=False)
    kra.fit(ctx, b, B, fetch=False)
    A2.close()
    ctx.synchronize()
    assert np.abs(ctx.fit_result(0, W) - ref[0]).max() <= _tol(ref[0])
    assert np.abs(ctx.fit_result(1, W) - ref[1]).max() <= _tol(ref[1])


def test_deferred_failure_of_a_group_member_surfaces_at_synchronize(ctx, G, sets):
    st = sets["headline"]
    z = np.zeros((NS, 6))
    u = np.random.default_rng(0).uniform(-1, 1, (NS, 3))
    bad = kra.Snapshots(ctx, z, z, u)            # all-zero states: the Gram matrix is singular
    kra.fit(ctx, st.b, st.snaps[0], fetch=False)
    kra.fit(ctx, st.b, bad, fetch=False)
    kra.fit(ctx, st.b, st.snaps[2], fetch=False)
    with pytest.raises(kra.KoopmanHipError) as e:
        ctx.synchronize()
    assert e.value.code == F.KP_ERR_NOT_SPD
    ctx.synchronize()                            # the sticky flag was cleared
    for q, i in ((0, 0), (2, 2)):                # the members beside the failing one are whole
        assert np.abs(ctx.fit_result(q, st.W) - st.Kref[i]).max() <= _tol(st.Kref[i])


_SUB = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import koopman_realizations_amd as kra
from oracle import koopman_oracle as ko
from conftest import synth_pairs
from test_gpu_fit import make_basis
what, out = sys.argv[2], sys.argv[3]
ctx = kra.Context(0)
res = {}
if what == "lone":
    for name, (nz, m, deg) in (("headline", (6, 3, 3)), ("m2", (3, 2, 2)), ("m1", (3, 1, 2))):
        b = kra.Basis(ctx, "bilinear", nz, m, [("poly", kra.poly_exponent_table(nz, deg)[nz:])])
        p = synth_pairs(4099, nz, m, seed=900)
        s = kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"])
        kra.fit(ctx, b, s, fetch=False)
        res[name] = ctx.fit_result(0, b.W)
else:
    for name, mt, dim_red in (("pcs", "bilinear", True), ("linear", "linear", False)):
        sets = [synth_pairs(4099, seed=910 + i) for i in range(3)]
        dic = ko.build_dictionary(mt, 6, 3, ["poly"], [3], sets[0], dim_red, [])
        b = make_basis(ctx, dic)
        snaps = [kra.Snapshots(ctx, p["alpha"], p["beta"], p["u"]) for p in sets]
        Kref = [kra.fit(ctx, b, s)[0] for s in snaps]
        for s in snaps:
            kra.fit(ctx, b, s, fetch=False)
        ctx.synchronize()
        for i in range(3):
            K = ctx.fit_result(i, b.W)
            assert np.abs(K - Kref[i]).max() <= 1e-11 * np.abs(Kref[i]).max(), (name, i)
            res["%s%d" % (name, i)] = K
np.savez(out, **res)
print("SUB_OK")
"""


def _run_sub(what, out, group):
    env = {k: v for k, v in os.environ.items() if k != "KP_GRAM_GROUP"}
    if group is not None:
        env["KP_GRAM_GROUP"] = str(group)
    r = subprocess.run([sys.executable, "-c", _SUB, ROOT, what, out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SUB_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)


@pytest.mark.parametrize("what", ["lone", "nongroupable"])
def test_group_of_one_and_fits_that_never_group_equal_the_ungrouped_pipeline_bitwise(tmp_path, what):
    """A lone pipelined fit (the group has one member) and pipelined fits of dictionaries that never group (a dim_red
    dictionary, a linear poly-3 one; three each, compared with their synchronous fits inside the child) give the same bits with
    the default group size and with KP_GRAM_GROUP=1 - the variable is read once, hence a process each."""
    a = _run_sub(what, str(tmp_path / "default.npz"), None)
    b = _run_sub(what, str(tmp_path / "one.npz"), 1)
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 3
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
