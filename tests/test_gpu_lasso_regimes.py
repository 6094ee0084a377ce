"""The iteration kernels of the L1-constrained fit (csrc/kp_lasso.hip) in every regime of their dispatch, with the two masks
that hide their errors off and with the defaults.  kp_timer_get(27) (include/koopman_hip.h) tells which kernels a batch ran,
and every test asserts the bits it is about.

Problems, well conditioned on purpose so that the plain projected-gradient iteration converges in a few hundred steps:
G = P'P / Ns with P standard normal (Ns = 8 W, W), C standard normal (W, ncols), budgets as fractions of |K_LS|_1.
Yardsticks, the project's own (tests/test_gpu_lasso.py): the budget met to 1e-9 relative; lasso_kkt_residual <= 1e-8 max|C|;
where n = W ncols <= 5000 also the exact active-set optimum of the oracle (koopman_lasso_path) to 1e-8 max|K|.  The observed
residuals are printed.

(a) pure iteration - a fresh process with KP_LASSO_PATH_AFTER=-1 and KP_LASSO_NO_POLISH=1, so neither the homotopy nor the
    active-set polish can repair what the projection or the product got wrong (kp_timer_get(11) == 0).  One value per call
    and W = 32: wpv = 32 workgroups per value, and each column count puts ceil(ceil(n / 32) / 1024) into one template of
    kp_lasso_project_kernel<EPT>, on either side of every threshold.  Slice edges: n < wpv (most workgroups own nothing),
    slices of 3 with a short last one, n = 1023.
(b) the multi-launch form (kp_lasso_v / newton / final kernels, reductions finished by last_block) under KP_LASSO_NO_FUSED=1 in
    a second process: one workgroup per value, four, and the 256-workgroup cap with strided blocks.  (a) and (b) agree to 1e-9
    max|K| on the shapes they share.
(c) the defaults in process on the shapes of (a), five budgets per call, one of them inactive: retirement, compaction and the
    hand-over to the homotopy.
(d) more running values than CUs: the batch starts in the multi-launch form and crosses into the one-launch form as values
    retire; retirement passes of more than 48 copies.  With the defaults, and in a child without the active-set rounds.
(e) the product kernels through the solver: the tiled kernel (RA = 8) while all values run, the small one once enough retired."""
import functools

import numpy as np
import pytest

from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from _lasso_child import in_fresh_process

pytestmark = pytest.mark.gpu

PROJ_BITS = sum(F.LASSO_RAN_EPT.values())
# (a), W = 32, one value: ncols -> the template ceil(ceil(32 ncols / 32) / 1024) = 4, 5, 8, 9, 16, 17, 24, 25 lands in
EPT_SHAPES = [(4096, 4), (4097, 8), (8192, 8), (8193, 16), (16384, 16), (16385, 24), (24576, 24), (24577, 0)]
EDGE_SHAPES = [(5, 1), (7, 11), (33, 31)]                    # n = 5 < wpv; n = 77: slices of 3, a short last one; n = 1023
SHARED_SHAPES = [(6, 10), (25, 40)]                          # n = 60, n = 1000: shapes of (a) and of (b)
MULTI_ONLY_SHAPES = [(35, 2000)]                             # n = 70 000: the cap of 256 workgroups, strided blocks
PURE_SHAPES = [(32, nc) for nc, _ in EPT_SHAPES] + EDGE_SHAPES + SHARED_SHAPES
MULTI_SHAPES = SHARED_SHAPES + MULTI_ONLY_SHAPES
PURE_FRACTIONS = (0.5, 0.05)
DEFAULT_FRACTIONS = (1.5, 0.9, 0.5, 0.1, 0.01)
EXACT_MAX_N = 5000


def expected_ept(n, running, cus):
    """The template kp_lasso_batch_dev launches: wpv = min(32, CUs / running values) workgroups per value, up to EPT elements
    of a slice per thread of 1024."""
    wpv = max(1, min(32, cus // running))
    ept = -(-(-(-n // wpv)) // 1024)
    return 0 if ept > 24 else 4 if ept <= 4 else 8 if ept <= 8 else 16 if ept <= 16 else 24


@functools.lru_cache(maxsize=None)
def problem(W, ncols, seed=0):
    rng = np.random.default_rng([seed, W, ncols])
    P = rng.standard_normal((8 * W, W))
    G = P.T @ P / (8 * W)
    G = (G + G.T) / 2
    C = rng.standard_normal((W, ncols))
    l1 = float(np.abs(np.linalg.solve(G, C)).sum())
    for a in (G, C):
        a.setflags(write=False)
    return G, C, l1


@functools.lru_cache(maxsize=None)
def exact(W, ncols, t, seed=0):
    G, C, _ = problem(W, ncols, seed)
    K = ko.koopman_lasso_path(G, C, t)[0]
    K.setflags(write=False)
    return K


def check_value(regime, W, ncols, f, K):
    """Budget, optimality conditions and (small problems) the exact optimum; returns the KKT residual relative to its bound."""
    G, C, l1 = problem(W, ncols)
    t = f * l1
    assert K.shape == (W, ncols) and np.isfinite(K).all(), (regime, W, ncols, f)
    assert abs(np.abs(K).sum() - t) <= 1e-9 * t, (regime, W, ncols, f, np.abs(K).sum() / t)
    rel = ko.lasso_kkt_residual(G, C, K, t) / (1e-8 * np.abs(C).max())
    line = f"lasso_regimes {regime}: W {W} ncols {ncols} budget {f:.4g}: kkt / (1e-8 max|C|) = {rel:.3e}"
    if W * ncols <= EXACT_MAX_N:
        Ke = exact(W, ncols, t)
        dk = np.abs(K - Ke).max() / (1e-8 * np.abs(Ke).max())
        line += f", |K - exact| / (1e-8 max|K|) = {dk:.3e}"
        print(line)
        assert dk <= 1.0, (regime, W, ncols, f, dk)
    else:
        print(line)
    assert rel <= 1.0, (regime, W, ncols, f, rel)
    return rel


@pytest.fixture(scope="module")
def cus(ctx):
    n = ctx.info()["num_cu"]
    assert n >= 32                                           # wpv = 32 for a lone value
    return n


# ---- (a) pure iteration ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pure():
    probs = []
    for W, nc in PURE_SHAPES:
        G, C, l1 = problem(W, nc)
        probs.append((G, C, [[f * l1] for f in PURE_FRACTIONS]))
    out = in_fresh_process(probs, {"KP_LASSO_PATH_AFTER": "-1", "KP_LASSO_NO_POLISH": "1"})
    return dict(zip(PURE_SHAPES, out))


@pytest.mark.parametrize("W,ncols", PURE_SHAPES, ids=lambda v: str(v))
def test_pure_iteration_in_every_projection_template(pure, cus, W, ncols):
    o = pure[(W, ncols)]
    want = F.LASSO_RAN_EPT[expected_ept(W * ncols, 1, cus)] | F.LASSO_RAN_SMALL          # W < 48: the small product kernel
    if W == 32:
        assert expected_ept(W * ncols, 1, cus) == dict(EPT_SHAPES)[ncols]
    for c, f in enumerate(PURE_FRACTIONS):
        assert o["ms"][c] == 0.0                                                         # no homotopy
        assert int(o["mask"][c]) == want, (f, hex(int(o["mask"][c])), hex(want))
        assert o["it"][c, 0] > 0
        check_value("(a) pure, EPT %d" % expected_ept(W * ncols, 1, cus), W, ncols, f, o["K"][c, 0])


# ---- (b) multi-launch form ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def multi():
    probs = []
    for W, nc in MULTI_SHAPES:
        G, C, l1 = problem(W, nc)
        probs.append((G, C, [[f * l1] for f in PURE_FRACTIONS]))
    out = in_fresh_process(probs, {"KP_LASSO_PATH_AFTER": "-1", "KP_LASSO_NO_POLISH": "1", "KP_LASSO_NO_FUSED": "1"})
    return dict(zip(MULTI_SHAPES, out))


@pytest.mark.parametrize("W,ncols", MULTI_SHAPES, ids=lambda v: str(v))
def test_multi_launch_form(multi, W, ncols):
    o = multi[(W, ncols)]
    assert -(-W * ncols // 256) == {60: 1, 1000: 4, 70000: 274}[W * ncols]               # workgroups per value, capped at 256
    for c, f in enumerate(PURE_FRACTIONS):
        assert o["ms"][c] == 0.0
        assert int(o["mask"][c]) == F.LASSO_RAN_MULTI | F.LASSO_RAN_SMALL, hex(int(o["mask"][c]))      # no projection bit
        assert o["it"][c, 0] > 0
        check_value("(b) multi-launch", W, ncols, f, o["K"][c, 0])


@pytest.mark.parametrize("W,ncols", SHARED_SHAPES, ids=lambda v: str(v))
def test_one_launch_and_multi_launch_forms_agree(pure, multi, W, ncols):
    for c, f in enumerate(PURE_FRACTIONS):
        Ka, Kb = pure[(W, ncols)]["K"][c, 0], multi[(W, ncols)]["K"][c, 0]
        d = np.abs(Ka - Kb).max() / np.abs(Ka).max()
        print(f"lasso_regimes (a) against (b): W {W} ncols {ncols} budget {f}: max |Ka - Kb| / max|K| = {d:.3e}")
        assert d <= 1e-9, (W, ncols, f, d)


# ---- (c) defaults -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,ncols", [(32, nc) for nc, _ in EPT_SHAPES] + EDGE_SHAPES, ids=lambda v: str(v))
def test_defaults_on_the_same_shapes(ctx, cus, W, ncols):
    G, C, l1 = problem(W, ncols)
    Kls = ctx.fit_solve(G, C)
    Ks, iters = ctx.fit_lasso_batch(G, C, np.array(DEFAULT_FRACTIONS) * l1)
    mask = int(ctx.timer(F.TIMER_LASSO_KERNELS))
    assert iters[0] == 0 and np.array_equal(Ks[0], Kls)                                  # inactive: the least-squares answer, bit for bit
    # four running values: still 32 workgroups each, so the template of (a); W < 48: the small product kernel
    assert mask == F.LASSO_RAN_EPT[expected_ept(W * ncols, 4, cus)] | F.LASSO_RAN_SMALL, hex(mask)
    assert expected_ept(W * ncols, 4, cus) == expected_ept(W * ncols, 1, cus)
    for f, K, it in zip(DEFAULT_FRACTIONS[1:], Ks[1:], iters[1:]):
        assert it > 0
        check_value("(c) defaults", W, ncols, f, K)


# ---- (d) more running values than CUs ----------------------------------------------------------------------------------------
# With the defaults the active-set polish ends almost every value of this small problem at the first check (iteration 4), while
# all of them still run in the multi-launch form: of the seeds 0 ... 149 of problem(12, 5, seed) only seed 41 leaves a value
# running behind it on a device of 256 CUs, which then goes on in the one-launch form.  The same batch therefore also runs in
# a child under KP_LASSO_ROUNDS=0 (the polish without its active-set rounds): there some forty values are still running behind
# the first check and go on in the one-launch form, so the change-over does not hang on one value.  (With the masks of (a)
# off the values of this batch all converge within one check of each other, and the batch ends in the form it began in.)
MANY_SHAPE, MANY_SEED = (12, 5), 41


def many_fractions(cus):
    """CUs + 44 active budgets, log-spaced, and two inactive ones in the middle of the list; their positions."""
    fr = list(np.geomspace(0.02, 0.95, cus + 44))
    mid = len(fr) // 2
    fr[mid:mid] = [1.5, 2.0]
    return fr, (mid, mid + 1)


def check_many(regime, fr, inactive, Ks, iters, Kls):
    W, ncols = MANY_SHAPE
    G, C, l1 = problem(W, ncols, MANY_SEED)
    worst = worst_k = 0.0
    for i, (f, K, it) in enumerate(zip(fr, Ks, iters)):
        if i in inactive:
            assert f > 1.0 and it == 0 and np.array_equal(K, Kls)                        # the least-squares answer, bit for bit
            continue
        assert it > 0
        t = f * l1
        assert abs(np.abs(K).sum() - t) <= 1e-9 * t, (regime, f, np.abs(K).sum() / t)
        rel = ko.lasso_kkt_residual(G, C, K, t) / (1e-8 * np.abs(C).max())
        Ke = exact(W, ncols, t, MANY_SEED)
        dk = np.abs(K - Ke).max() / (1e-8 * np.abs(Ke).max())
        worst, worst_k = max(worst, rel), max(worst_k, dk)
        assert rel <= 1.0 and dk <= 1.0, (regime, f, rel, dk)
    spent = dict(zip(*[x.tolist() for x in np.unique(iters, return_counts=True)]))
    print(f"lasso_regimes {regime}: {len(fr) - 2} running values: largest kkt / (1e-8 max|C|) = {worst:.3e}, largest |K - exact| / (1e-8 max|K|) = "
          f"{worst_k:.3e}; iterations spent: values {spent}")


def test_more_values_than_cus_changes_over_to_the_one_launch_form(ctx, cus):
    W, ncols = MANY_SHAPE
    G, C, l1 = problem(W, ncols, MANY_SEED)
    fr, inactive = many_fractions(cus)
    Kls = ctx.fit_solve(G, C)
    Ks, iters = ctx.fit_lasso_batch(G, C, np.array(fr) * l1)
    mask = int(ctx.timer(F.TIMER_LASSO_KERNELS))
    check_many("(d) defaults, mask %s" % hex(mask), fr, inactive, Ks, iters, Kls)
    assert mask & F.LASSO_RAN_MULTI and mask & PROJ_BITS, hex(mask)                      # started in one form, went on in the other
    assert mask & PROJ_BITS == F.LASSO_RAN_EPT[4] and mask & F.LASSO_RAN_SMALL and not mask & F.LASSO_RAN_TILED, hex(mask)


def test_more_values_than_cus_without_active_set_rounds(ctx, cus):
    W, ncols = MANY_SHAPE
    G, C, l1 = problem(W, ncols, MANY_SEED)
    fr, inactive = many_fractions(cus)
    o = in_fresh_process([(G, C, [np.array(fr) * l1])], {"KP_LASSO_ROUNDS": "0"}, timeout=120)[0]
    mask, iters = int(o["mask"][0]), o["it"][0]
    check_many("(d) one-shot polish, mask %s" % hex(mask), fr, inactive, o["K"][0], iters, ctx.fit_solve(G, C))
    assert mask == F.LASSO_RAN_MULTI | F.LASSO_RAN_EPT[4] | F.LASSO_RAN_SMALL, hex(mask)
    later = int((iters > 4).sum())                                                       # values that went on in the one-launch form
    assert 10 <= later <= cus, later


# ---- (e) product regimes through the solver ------------------------------------------------------------------------------------
def test_solver_runs_the_tiled_product_and_then_the_small_one(ctx):
    W, ncols, nv = 125, 80, 40
    assert nv * ncols * -(-W // 16) > 19000                                              # 3200 columns > 2375
    G, C, l1 = problem(W, ncols)
    fr = np.geomspace(0.02, 0.95, nv)
    Ks, iters = ctx.fit_lasso_batch(G, C, fr * l1)
    mask = int(ctx.timer(F.TIMER_LASSO_KERNELS))
    print(f"lasso_regimes (e): iterations spent -> values {dict(zip(*np.unique(iters, return_counts=True)))}, mask {hex(mask)}, homotopy {ctx.timer(11):.3f} ms")
    assert mask & F.LASSO_RAN_TILED and mask & F.LASSO_RAN_RA[8] and mask & sum(F.LASSO_RAN_RB.values()), hex(mask)
    assert not mask & (sum(F.LASSO_RAN_RA.values()) - F.LASSO_RAN_RA[8]), hex(mask)
    assert mask & F.LASSO_RAN_SMALL, hex(mask)                                           # ... as values retire
    worst = max(check_value("(e) tiled, then small", W, ncols, f, K) for f, K in zip(fr, Ks))
    print(f"lasso_regimes (e): largest kkt / (1e-8 max|C|) = {worst:.3e}, mask {hex(mask)}")
