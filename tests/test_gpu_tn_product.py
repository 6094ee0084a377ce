"""The TN product of the wide path (csrc/kp_tn_gemm.h: C = beta C + alpha (diag(wa wb) A)' B) alone, through kp_tn_product, in
every tile form, staging path, contraction split and epilogue, with the upper-tiles rule and with row weights.

Reference: numpy.longdouble, ref = beta C0 + alpha (A (wa wb)[:, None])' B; A, B, the weights and C0 uniform in [-0.5, 0.5] from
fixed seeds, built per case and dropped.
Tolerance, derived and not measured, entry by entry:
    |C - ref| <= (2 K + 8) eps (|alpha| (|A| |wa wb|)' |B| + |beta| |C0|)
2 K eps is the forward bound of a length-K f64 dot product in any summation order (it covers the order of the splits and of the
4x4x4 MFMA blocks), + 8 the two roundings of the weights and the alpha / beta epilogue.  The largest |C - ref| / bound of every
test is printed.

Every case also requires:
 (a) `ran` names the expected form, staging path and split count (expected_vec, splits_that_run below restate the launcher's
     small formulas; tests/test_tn_abi.py checks them against the tables here);
 (b) rows M ... ldc - 1 of every column of C come back bitwise as uploaded (they are NaN);
 (c) rows K ... ld - 1 of A and B are NaN, and nothing of that may reach the result: the masking of the last contraction block
     and the k_hi of the last split;
 (d) with beta == 0 all of C0 is NaN and the result must be free of NaN: the epilogue must not read C;
 (e) with tri: every element i <= j meets the bound; every element i > j meets the bound (its tile ran) or is bitwise what was
     uploaded, nothing else; with two or more row tiles at least one element is untouched.  That holds for any tile size, and
     fails when the product's dealing loop, tng_count_tiles and the reduction's skip rule disagree.

Left out on purpose: that the bound on the leading dimensions (32-bit tile offsets) is TIGHT would need a 4 GB operand; only the
refusal at the bound is tested."""
import ctypes as C

import numpy as np
import pytest

from koopman_realizations_amd import _ffi as F

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SMALL = F.TN_FORM_SMALL


def tile(code):
    return (64, 64) if code == SMALL else F.TN_SHAPES[code]


def splits_that_run(K, ns):
    """kp_tn_gemm: a split's contraction range is a multiple of 16, and the splits that are left with nothing do not run."""
    if ns <= 1:
        return 1
    kper = max(16, -(-(-(-K // ns)) // 16) * 16)
    return -(-K // kper)


def expected_vec(code, lda, ldb, misalign):
    """tng_launch_cfg: the 16-byte staging needs aligned operands and even leading dimensions; form 2 (<8, 6, 8>) stages 3 rows of
    B per thread and has no such instantiation."""
    return int(not misalign and lda % 2 == 0 and ldb % 2 == 0 and code != 2)


# (K, splits asked for) -> splits that run (tests/test_tn_abi.py: splits_that_run gives these)
SPLITS = {(40, 2): 2, (40, 3): 3, (40, 5): 3, (100, 2): 2, (100, 3): 3, (100, 5): 4, (257, 2): 2, (257, 3): 3, (257, 5): 5}
# staging modes of the contraction-length cases: (what is added to K for the leading dimensions, KP_TN_MISALIGN) -> vec for
# even K, vec for odd K (tests/test_tn_abi.py: expected_vec gives these)
STAGING = {(0, False): (1, 0), (6, False): (1, 0), (1, False): (0, 1), (7, False): (0, 1),
           (0, True): (0, 0), (6, True): (0, 0), (1, True): (0, 0), (7, True): (0, 0)}

C0_NAN = 0x7ff8000000000c0c
_ratios = []


@pytest.fixture(autouse=True)
def _print_worst_ratio(request):
    _ratios.clear()
    yield
    if _ratios:
        print(f"tn_product {request.node.name}: {len(_ratios)} products, max |C - ref| / bound = {max(_ratios):.3e}")


def _bits(X):
    return np.ascontiguousarray(X).view(np.int64)


def _run(ctx, M, N, K, *, lda=None, ldb=None, ldc=None, alpha=1.0, beta=0.0, tri=0, nsplit=1, wa=False, wb=False, form=-1, flags=0,
         want_form=None):
    """One product against the extended-precision reference, with the checks (a) - (e).  Returns (C as it came back, ran)."""
    same, mirror = bool(flags & F.TN_SAME), bool(flags & F.TN_MIRROR)
    lda = K if lda is None else lda
    ldb = lda if same else K if ldb is None else ldb
    ldc = M if ldc is None else ldc
    label = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, alpha=alpha, beta=beta, tri=tri, nsplit=nsplit, wa=wa, wb=wb, form=form, flags=flags)
    rng = np.random.default_rng([M, N, K, lda, ldb, ldc, nsplit, int(wa) + 2 * int(wb)])         # (not the flags, tri, form: those cases are compared bit for bit)
    A = np.full((lda, M), np.nan, order="F")
    A[:K] = rng.uniform(-0.5, 0.5, (K, M))
    if same:
        B = None
    else:
        B = np.full((ldb, N), np.nan, order="F")
        B[:K] = rng.uniform(-0.5, 0.5, (K, N))
    va = rng.uniform(-0.5, 0.5, K) if wa else None
    vb = rng.uniform(-0.5, 0.5, K) if wb else None
    C0 = np.zeros((ldc, N), order="F")
    C0.view(np.int64)[...] = C0_NAN                         # (a NaN of its own: one that leaks from the padding of A or B is another)
    if beta != 0.0:
        C0[:M] = rng.uniform(-0.5, 0.5, (M, N))
    w = (np.ones(K, LD) if va is None else va.astype(LD)) * (np.ones(K, LD) if vb is None else vb.astype(LD))
    Ak, Bk = A[:K].astype(LD), (A if same else B)[:K].astype(LD)
    ref = LD(alpha) * ((Ak * w[:, None]).T @ Bk)
    bound = abs(LD(alpha)) * ((np.abs(Ak) * np.abs(w)[:, None]).T @ np.abs(Bk))
    if beta != 0.0:
        ref += LD(beta) * C0[:M].astype(LD)
        bound += abs(LD(beta)) * np.abs(C0[:M]).astype(LD)
    bound *= (2 * K + 8) * LD(EPS)
    if mirror:                                              # the lower triangle is a copy of the upper one
        ref, bound = np.triu(ref) + np.triu(ref, 1).T, np.triu(bound) + np.triu(bound, 1).T

    Cm = C0.copy(order="F")
    ran = ctx.tn_product(A, B, Cm, K=K, alpha=alpha, beta=beta, tri=tri, nsplit=nsplit, wa=va, wb=vb, form=form, flags=flags)

    # (a)
    code, vec, ns = ran // F.TN_RAN_FORM, ran // F.TN_RAN_VEC % 10, ran % F.TN_RAN_VEC
    if M <= 64:
        assert code == SMALL, (label, ran)
    elif form >= 0:
        assert code == form, (label, ran)
    else:
        assert code in (0, 1), (label, ran)
    if want_form is not None:
        assert code == want_form, (label, ran)
    assert vec == expected_vec(code, lda, ldb, bool(flags & F.TN_MISALIGN)), (label, ran)
    assert ns == splits_that_run(K, nsplit), (label, ran)
    # (b)
    assert np.array_equal(_bits(Cm[M:]), _bits(C0[M:])), (label, "rows beyond M were written")
    # the bound; (c), (d): a NaN from the padding, from C0 or from a partial nobody wrote fails it
    ratio = np.abs(Cm[:M].astype(LD) - ref) / bound
    ok = ratio <= 1.0                                        # (False for NaN)
    if not tri or mirror:
        assert ok.all(), (label, ran, int((~ok).sum()), "elements miss the bound; first at", tuple(np.argwhere(~ok)[0]))
        _ratios.append(float(ratio.max()))
    else:
        # (e)
        i, j = np.indices((M, N))
        upper = i <= j
        untouched = ~upper & (_bits(Cm[:M]) == _bits(C0[:M]))
        bad = ~ok & ~untouched
        assert not bad.any(), (label, ran, int(bad.sum()), "elements are neither right nor untouched; first at", tuple(np.argwhere(bad)[0]))
        if -(-M // tile(code)[0]) >= 2:
            assert untouched.any(), (label, ran, "no tile was skipped")
        _ratios.append(float(ratio[ok].max()))
    return Cm, ran


# ---- forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 64])
def test_small_form(ctx, M):
    """64 x 64 tiles; N = 8 * 64 + 1 is a ninth column tile, where the XCD order wraps.  Forcing a form is ignored at M <= 64."""
    for N in (1, 63, 64, 65, 8 * 64 + 1):
        _run(ctx, M, N, 33, lda=34, ldb=34, ldc=M + 1, want_form=SMALL)
        _run(ctx, M, N, 33, form=2, want_form=SMALL)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_forced_form(ctx, form):
    """A partial first tile, exactly one tile and a second row tile of one row; one column, one column tile, one column more, and a
    ninth column tile."""
    TM, TN = F.TN_SHAPES[form]
    for M in (65, TM, TM + 1):
        for N in (1, TN, TN + 1, 8 * TN + 1):
            _run(ctx, M, N, 33, lda=34, ldb=34, ldc=M + 1, form=form)
            _run(ctx, M, N, 16, alpha=-1.0, beta=1.0, form=form, flags=F.TN_MISALIGN)


def test_form_by_shape(ctx):
    seen = set()
    for M, N in ((65, 65), (129, 97), (200, 200), (300, 520)):
        seen.add(_run(ctx, M, N, 32)[1])
    print("tn_product form = -1 at M > 64: ran", sorted(seen))
    for M, N in ((1, 1), (64, 300)):
        ran = _run(ctx, M, N, 32, want_form=SMALL)[1]
        print(f"tn_product form = -1 at M = {M}: ran {ran}")


# ---- contraction length and staging path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 15, 16, 17, 31, 32, 33, 48])
def test_contraction_length_in_every_staging_mode(ctx, K):
    """No full block, exactly one, a partial block that ends on an odd index (the second element of a 16-byte pair lies beyond K),
    an even and an odd number of blocks; leading dimensions K, K + 6 and the next even / odd ones, the padding NaN; 16-byte
    staging, 8-byte staging by an odd leading dimension and by misaligned operands."""
    for M, N, form in ((63, 65, -1), (129, 65, 0)):
        for (pad, mis), vecs in STAGING.items():
            ld = K + pad
            if mis and ld % 2:
                continue                                    # (misalignment is the reason for the 8-byte path only at an even ld)
            ran = _run(ctx, M, N, K, lda=ld, ldb=ld, ldc=M + 2, form=form, flags=F.TN_MISALIGN if mis else 0)[1]
            assert ran // F.TN_RAN_VEC % 10 == vecs[K % 2], (K, ld, mis, ran)


def test_one_odd_leading_dimension_is_enough_for_the_8_byte_path(ctx):
    for lda, ldb, vec in ((34, 34, 1), (35, 34, 0), (34, 35, 0), (35, 35, 0)):
        for M, form in ((63, -1), (129, 0), (129, 1), (193, 3)):
            ran = _run(ctx, M, 70, 33, lda=lda, ldb=ldb, form=form)[1]
            assert ran // F.TN_RAN_VEC % 10 == vec, (lda, ldb, ran)
    assert _run(ctx, 257, 70, 33, lda=34, ldb=34, form=2)[1] // F.TN_RAN_VEC % 10 == 0


# ---- epilogue --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)])
def test_epilogue(ctx, alpha, beta):
    """In the product kernel (one split) and in the reduction (two), with C as wide as it is high and wider."""
    for M, N, form in ((63, 65, -1), (129, 65, 0), (129, 97, 1), (257, 97, 2), (193, 129, 3)):
        for ldc in (M, M + 3):
            for nsplit in (1, 2):
                _run(ctx, M, N, 40, ldc=ldc, alpha=alpha, beta=beta, nsplit=nsplit, form=form)


# ---- split-K -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [40, 100, 257])
@pytest.mark.parametrize("M,N,form", [(63, 65, -1), (129, 129, 0), (129, 129, 1)])
def test_split_k(ctx, M, N, form, K):
    """Splits asked for and splits that run (at K = 40 five collapse to three, the last with 8 indices; at K = 257 the fifth has
    one), with and without the upper-tiles rule in product and reduction, partial sums added to C or not; twice the same bits."""
    for nsplit in (2, 3, 5):
        for tri in (0, 1):
            for beta in (0.0, 1.0):
                for ld in (K, K + 1):
                    C1, ran = _run(ctx, M, N, K, lda=ld, ldb=ld, ldc=M + 3, beta=beta, tri=tri, nsplit=nsplit, form=form)
                    assert ran % F.TN_RAN_VEC == SPLITS[K, nsplit], (K, nsplit, ran)
                C2, _ = _run(ctx, M, N, K, lda=ld, ldb=ld, ldc=M + 3, beta=beta, tri=tri, nsplit=nsplit, form=form)
                assert np.array_equal(_bits(C1), _bits(C2)), (M, N, K, nsplit, tri, beta)


# ---- upper tiles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("M,N", [(200, 200), (300, 300), (200, 248)])
def test_upper_tiles(ctx, M, N, form):
    """Square, and the solve's [A22 | C_rest] with N > M.  The i <= j part does not depend on the rule, bit for bit."""
    for K, nsplit in ((33, 1), (40, 2)):
        for beta in (0.0, 1.0):
            Ct, _ = _run(ctx, M, N, K, lda=K + 1, ldb=K + 1, ldc=M + 1, alpha=-1.0, beta=beta, tri=1, nsplit=nsplit, form=form)
            Cf, _ = _run(ctx, M, N, K, lda=K + 1, ldb=K + 1, ldc=M + 1, alpha=-1.0, beta=beta, tri=0, nsplit=nsplit, form=form)
            i, j = np.indices((M, N))
            assert np.array_equal(_bits(Ct[:M])[i <= j], _bits(Cf[:M])[i <= j]), (M, N, form, K, nsplit, beta)


@pytest.mark.parametrize("M", [40, 64])
def test_upper_tiles_of_the_small_form_skip_nothing(ctx, M):
    """One row tile: every tile meets the upper triangle, but the per-XCD dealing runs, with a tile count (9) that is no multiple of 8."""
    for nsplit, K in ((1, 33), (3, 40)):
        Cm, _ = _run(ctx, M, 8 * 64 + 1, K, tri=1, nsplit=nsplit, want_form=SMALL)
        assert not np.isnan(Cm).any()


@pytest.mark.parametrize("form", [-1, 0, 1, 2, 3])
def test_same_operand_upper_tiles_and_mirror_give_a_symmetric_matrix(ctx, form):
    for M in (63, 200, 300):
        for K, nsplit, ld in ((33, 1, 34), (40, 2, 41), (100, 3, 100)):
            for mis in (0, F.TN_MISALIGN):
                Cm, _ = _run(ctx, M, M, K, lda=ld, tri=1, nsplit=nsplit, form=form, flags=F.TN_SAME | F.TN_MIRROR | mis)
                assert not np.isnan(Cm).any() and np.array_equal(Cm, Cm.T), (M, K, nsplit, form)


# ---- weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,nsplit", [(33, 1), (100, 3)])
@pytest.mark.parametrize("wa,wb", [(True, False), (False, True), (True, True)])
def test_weights(ctx, wa, wb, K, nsplit):
    """Weights of the contraction index in both staging paths, in a partial last block, beyond the first split (k_lo offsets
    them), with and without the upper-tiles rule, and with B = A as the Kronecker Gram matrices call the product."""
    for M, N, form in ((63, 63, -1), (129, 129, -1), (193, 193, 3)):
        for ld in (K + K % 2, K + K % 2 + 1):                            # even: 16-byte staging; odd: 8-byte
            for tri in (0, 1):
                for flags in (0, F.TN_SAME, F.TN_MISALIGN):
                    _run(ctx, M, N, K, lda=ld, ldb=ld, ldc=M + 1, beta=1.0, tri=tri, nsplit=nsplit, wa=wa, wb=wb, form=form, flags=flags)


# ---- the callers' own shapes, reduced ---------------------------------------------------------------------------------------
def test_block_substitution_shapes(ctx):
    """kp_solve.hip, wide_substitute with n = 96, b = 16: the backward step at k0 = 48 (C[0:48] -= G[48:64, 0:48]' C[48:64]) and the
    forward step at k0 = 16 (R = 64 rows below the block); the operands lie in the middle of n-row matrices, the NaN padding
    plays the rest of them."""
    _run(ctx, 48, 16, 16, lda=96, ldb=96, ldc=96, alpha=-1.0, beta=1.0)
    _run(ctx, 64, 16, 16, lda=96, ldb=96, ldc=96, alpha=-1.0, beta=1.0)
    _run(ctx, 80, 80 + 16, 16, lda=96, ldb=96, ldc=96, alpha=-1.0, beta=1.0, tri=1)       # trailing update with [A22 | C_rest]


@pytest.mark.parametrize("n", [1, 2, 37, 64, 65, 129, 250])
def test_logm_shapes(ctx, n):
    """kp_logm: M = N = K = n, dense leading dimensions, one split, C overwritten."""
    _run(ctx, n, n, n)


# ---- kp_mirror_upper_kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_mirror_upper(ctx, n):
    for ldc in (n, n + 5):
        plain, _ = _run(ctx, n, n, 20, ldc=ldc)
        mirrored, _ = _run(ctx, n, n, 20, ldc=ldc, flags=F.TN_MIRROR)
        i, j = np.indices((n, n))
        P, Q = _bits(plain[:n]), _bits(mirrored[:n])
        assert np.array_equal(Q[i <= j], P[i <= j]), (n, ldc, "the upper triangle or the diagonal changed")
        assert np.array_equal(Q[i > j], Q.T[i > j]), (n, ldc, "the lower triangle is not the transpose of the upper one")
        assert np.array_equal(_bits(mirrored[n:]), _bits(plain[n:]))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _raw(ctx, A, lda, B, ldb, M, N, K, Cm, ldc, nsplit=1, form=-1, flags=0, tri=0):
    ran = C.c_int(-7)
    rc = F.lib().kp_tn_product(ctx._h, F.dptr(A), lda, F.dptr(B), ldb, M, N, K, F.dptr(Cm), ldc, 1.0, 0.0, tri, nsplit, None, None, form, flags, C.byref(ran))
    return rc, ran.value


def test_bad_arguments_are_refused(ctx):
    A, B = np.ones((8, 4), order="F"), np.ones((8, 4), order="F")
    C0 = np.full((4, 4), 3.0, order="F")
    Cm = C0.copy(order="F")
    ok = dict(A=A, lda=8, B=B, ldb=8, M=4, N=4, K=8, Cm=Cm, ldc=4)
    assert _raw(ctx, **ok)[0] == F.KP_OK and np.array_equal(Cm, np.full((4, 4), 8.0))
    bad = [dict(A=None), dict(Cm=None), dict(B=None), dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(lda=7), dict(ldb=7), dict(ldc=3),
           dict(form=-2), dict(form=4), dict(flags=8), dict(flags=F.TN_SAME | 16), dict(nsplit=0), dict(nsplit=65),
           dict(N=3, flags=F.TN_SAME), dict(N=3, flags=F.TN_MIRROR), dict(N=5, ldc=4, flags=F.TN_MIRROR), dict(ldb=10, flags=F.TN_SAME)]
    for change in bad:
        Cm[:] = C0
        rc, ran = _raw(ctx, **{**ok, **change})
        assert rc == F.KP_ERR_ARG and ran == -7, (change, rc, ran)
        assert np.array_equal(Cm, C0), change
    assert _raw(ctx, **{**ok, "B": None, "flags": F.TN_SAME})[0] == F.KP_OK             # B may be NULL when it is A


def test_leading_dimension_beyond_the_32_bit_offsets_is_refused(ctx):
    """256 lda 8 + K 8 reaches 2^32 at lda = 2^21: kp_tn_gemm refuses and C stays as uploaded.  (M = 1: only K doubles of A exist.)"""
    A, B = np.ones(8), np.ones((8, 1), order="F")
    C0 = np.full((1, 1), 3.0, order="F")
    Cm = C0.copy(order="F")
    rc, ran = _raw(ctx, A, 1 << 21, B, 8, 1, 1, 8, Cm, 1)
    assert rc not in (F.KP_OK,) and ran == -7 and np.array_equal(Cm, C0), (rc, ran, Cm)
    assert b"kp_tn_gemm" in F.lib().kp_last_error(ctx._h)
    rc, ran = _raw(ctx, B, 8, A, 1 << 21, 1, 1, 8, Cm, 1)                         # ... of either operand
    assert rc != F.KP_OK and np.array_equal(Cm, C0)
    rc, ran = _raw(ctx, A, (1 << 21) - 2, B, 8, 1, 1, 8, Cm, 1)                  # just below the bound the product runs
    assert rc == F.KP_OK and Cm[0, 0] == 8.0 and ran == F.TN_RAN_FORM * SMALL + F.TN_RAN_VEC + 1, (rc, ran, Cm)
