"""The product kernels of the lasso iteration (csrc/kp_symm_gemm.h) alone, through kp_symm_product, in every regime of their
dispatch: C = G X with G symmetric against the same product in extended precision.

Reference: G.astype(longdouble) @ X.astype(longdouble); G and X uniform in [-0.5, 0.5] from a fixed seed.
Tolerance, derived and not measured: |C - ref| <= 2 W eps (|G| @ |X|) entry by entry - the forward bound of a length-W f64 dot
product in any summation order (W eps / 2 per unit of |g|'|x| to first order), with room for the split-k halves of the small
kernel and the accumulation order of the 4x4x4 MFMA blocks.  Every case also requires that no NaN is left in C (the entry point
fills the device buffer with NaN before the launch: an element that no lane stored shows) and that `ran` names the kernel the
case is about.  The largest |C - ref| / bound of every case is printed.

Regimes: kp_symm_gemm2_kernel<RA, RB> at all 5 x 4 instantiations (RA = 4 ... 8 by W, RB forced by variant 10 + RB), with and
without a partial last contraction block, with an odd number of blocks, a partial second row tile, a last column tile narrower
than 16 RB and a ninth column tile (the XCD order wraps); the automatic dispatch on either side of its threshold
nc ceil(W / 16) > 19000; kp_symm_gemm_kernel at W not a multiple of 4, W <= 4 (an empty second split-k half), the largest W
its LDS holds (404) and column counts around its 32-column tile; kp_symm_gemm_naive_kernel at the first W beyond that.

Left out on purpose: the fall-back from the tiled kernel's 32-bit byte offsets (nc W 8 >= 2^32) needs a 4 GB operand, which is
not a test of a few seconds."""
import functools

import numpy as np
import pytest

from koopman_realizations_amd import _ffi as F

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def pick_ra(W):
    """sg2_pick_ra of csrc/kp_symm_gemm.h: the RA in 4 ... 8 with the least padded rows, ties to the larger tile."""
    wg = (W + 3) // 4
    best, best_pad = 8, 1 << 30
    for ra in range(8, 3, -1):
        pad = -(-wg // (4 * ra)) * 4 * ra
        if pad < best_pad:
            best, best_pad = ra, pad
    return best


@functools.lru_cache(maxsize=None)
def _G(W):
    A = np.random.default_rng(1000 + W).uniform(-0.5, 0.5, (W, W))
    G = np.triu(A) + np.triu(A, 1).T
    assert np.array_equal(G, G.T)
    return G


def _case(W, nc):
    """G, X, the extended-precision product and the entrywise bound.  Built per case and dropped: nothing the device wrote can
    reach it."""
    G = _G(W)
    X = np.random.default_rng(7 * W + 13 * nc).uniform(-0.5, 0.5, (W, nc))
    ref = G.astype(np.longdouble) @ X.astype(np.longdouble)
    bound = 2 * W * EPS * (np.abs(G) @ np.abs(X))
    return G, X, ref, bound


def _check(ctx, W, nc, variant, label):
    G, X, ref, bound = _case(W, nc)
    C, ran = ctx.symm_product(G, X, variant)
    assert C.shape == (W, nc)
    assert not np.isnan(C).any(), (label, W, nc, int(np.isnan(C).sum()))
    rel = float((np.abs(C.astype(np.longdouble) - ref) / bound).max())
    print(f"symm_product {label}: W {W} nc {nc} variant {variant} ran {ran}: max |C - ref| / bound = {rel:.3e}")
    assert rel <= 1.0, (label, W, nc, rel)
    return ran


# W: (RA, contraction blocks) - restated from sg2_pick_ra and ceil(W / 16); tests/test_lasso_abi.py checks them against pick_ra
TILED_W = {50: (4, 4), 64: (4, 4), 77: (5, 5), 93: (6, 6), 109: (7, 7), 125: (8, 8), 128: (8, 8), 130: (5, 9)}


@pytest.mark.parametrize("rb", [2, 3, 4, 6])
@pytest.mark.parametrize("W", sorted(TILED_W))
def test_tiled_kernel_with_forced_width(ctx, W, rb):
    """Narrower than a column tile, exactly one, a second tile of one column, and a ninth column tile."""
    for nc in (5, 16 * rb, 16 * rb + 1, 8 * 16 * rb + 3):
        ran = _check(ctx, W, nc, F.SYMM_TILED_RB + rb, "tiled")
        assert ran == F.SYMM_RAN_TILED + 10 * TILED_W[W][0] + rb, (W, nc, ran)


@pytest.mark.parametrize("W,nc", [(50, 4750), (125, 2375), (336, 904)])
def test_dispatch_by_shape_changes_kernel_at_its_threshold(ctx, W, nc):
    assert nc * -(-W // 16) <= 19000 < (nc + 1) * -(-W // 16)
    assert _check(ctx, W, nc, F.SYMM_BY_SHAPE, "by shape, small") == F.SYMM_RAN_SMALL
    ran = _check(ctx, W, nc + 1, F.SYMM_BY_SHAPE, "by shape, tiled")
    ra, rb = divmod(ran - F.SYMM_RAN_TILED, 10)
    assert ra == pick_ra(W) and rb in (2, 3, 4, 6), ran


@pytest.mark.parametrize("W", [1, 3, 4, 5, 17, 47, 60, 403, 404])
def test_small_kernel(ctx, W):
    for nc in (1, 31, 32, 33, 65):
        assert _check(ctx, W, nc, F.SYMM_BY_SHAPE, "small") == F.SYMM_RAN_SMALL
        assert _check(ctx, W, nc, F.SYMM_SMALL, "small, forced") == F.SYMM_RAN_SMALL


def test_naive_kernel_beyond_the_small_kernels_lds(ctx):
    assert 404 * 49 * 8 <= 156 * 1024 < 408 * 49 * 8                    # W = 405 stages 408 rows of 49 doubles
    for nc in (1, 33):
        assert _check(ctx, 405, nc, F.SYMM_BY_SHAPE, "naive") == F.SYMM_RAN_NAIVE
    ran = _check(ctx, 405, 731, F.SYMM_BY_SHAPE, "by shape, tiled")    # 731 x 26 = 19006 units
    ra, rb = divmod(ran - F.SYMM_RAN_TILED, 10)
    assert ra == pick_ra(405) and rb in (2, 3, 4, 6), ran


def test_bad_arguments_are_refused(ctx):
    import koopman_realizations_amd as kra
    G, X = _G(5), np.zeros((5, 2))
    with pytest.raises(kra.KoopmanHipError):
        ctx.symm_product(G, X, 7)
    with pytest.raises(ValueError):
        ctx.symm_product(_G(4), X)
