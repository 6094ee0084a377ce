"""The reference of the rollout tests in tests/test_gpu_model_kernel_regimes.py, checked on its own (no GPU): the helper's
constants are the kernel's, its case table reaches every regime of kp_rollout's host code that it names, and on every case
the long-double trajectory keeps a size at which a relative comparison means something while the plain float64 recurrence
stays two orders of magnitude inside the 1e-12 the device is held to.  A retuned kernel fails here instead of silently
leaving a regime uncovered; a seed that misses a condition is replaced in CASES, the conditions stay."""
import os
import re

import numpy as np
import pytest

import _rollout_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(src, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, src, re.M)
    assert m, name
    return int(m.group(1))


def test_the_helper_constants_are_the_kernels():
    with open(os.path.join(ROOT, "koopman-realizations_amd", "csrc", "kp_more.hip")) as f:
        src = f.read()
    assert _define(src, "RO_STAGE") == rr.RO_STAGE
    assert _define(src, "RO_TC") == rr.RO_TC
    # the host code sizes the chunks for 128 KB of LDS and takes the one-wave kernel up to N = 64
    assert "(128 * 1024 - lds_model) / ((size_t)(m + n_out) * 8)" in src
    assert re.search(r"if \(N <= 64\)\s*\n\s*hipLaunchKernelGGL\(kp_rollout_kernel<true>", src)


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_case_table_reaches_the_regime_it_names(name):
    bil, N, m, n_out, Ts, _, regime, _ = rr.CASES[name]
    got = rr.rollout_regime(N, m, bil, n_out)
    assert got == regime, (name, got)
    tcmax = got[3]
    # lengths on both sides of a chunk boundary, and one that needs a third chunk, wherever the case has several lengths
    if len(Ts) >= 3:
        assert {tcmax, tcmax + 1, 2 * tcmax + 1} <= set(Ts) or (tcmax == 256 and {256, 257} <= set(Ts)), (name, tcmax, Ts)


def test_case_table_covers_every_regime():
    regs = {name: rr.rollout_regime(c[1], c[2], c[0], c[3]) for name, c in rr.CASES.items()}
    N = {name: c[1] for name, c in rr.CASES.items()}
    assert any(r[0] and N[n] == 64 for n, r in regs.items()) and any(not r[0] and N[n] == 65 for n, r in regs.items())
    assert {(r[1], r[2]) for r in regs.values()} == {(True, True), (True, False), (False, False)}
    assert any(r[3] == rr.RO_TC for r in regs.values()) and any(r[3] < rr.RO_TC for r in regs.values())
    assert any(n > 256 for n in N.values())
    assert any(c[2] == 0 for c in rr.CASES.values())
    # the staging limits from both sides: the last staged A and the first unstaged one, B exactly at its limit and beyond it
    assert 90 * 90 <= rr.RO_STAGE < 91 * 91 and {90, 91} <= set(N.values())
    assert 64 * 64 + 64 * 64 * 2 == rr.RO_STAGE + rr.RO_STAGE // 2 and regs["e"][2] and not regs["d"][2]
    for name in ("a", "d", "g", "h_bil"):
        assert rr.CASES[name][7]


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_reference_keeps_its_size_and_float64_agrees(name):
    bil, N, m, n_out, Ts, _, _, batched = rr.CASES[name]
    T = max(Ts)
    for index in range(rr.BATCH if batched else 1):
        c = rr.case(name, T, index)
        Z = c["Z"]
        assert Z.dtype == np.longdouble and Z.shape == (T, N)
        norm = np.abs(Z).max(axis=1).astype(np.float64)
        Zd = rr.rollout_reference(c["A"], c["B"], c["z0"], c["U"], bil, dtype=np.float64)
        err = (np.abs(Zd - Z).max(axis=1).astype(np.float64) / norm).max()
        print("case %s model %d: T %d inf-norm %.3g ... %.3g, float64 against long double %.2e" % (name, index, T, norm.min(), norm.max(), err))
        assert 1e-2 <= norm.min() and norm.max() <= 1e2
        assert err <= 1e-13
    if batched:       # the members of a batch are distinct models
        c0, c1 = rr.case(name, T, 0), rr.case(name, T, 1)
        assert not np.array_equal(c0["A"], c1["A"]) and not np.array_equal(c0["U"], c1["U"])


def test_reference_is_the_recurrence():
    """The reference against a literal evaluation of two steps, linear and bilinear (B kron(I_m, z) u, Ksysid.m:1285-1295)."""
    rng = np.random.default_rng(3)
    N, m = 4, 2
    A = rng.standard_normal((N, N)); z0 = rng.standard_normal(N); U = rng.standard_normal((3, m))
    B = rng.standard_normal((N, m))
    Z = rr.rollout_reference(A, B, z0, U, False, dtype=np.float64)
    z1 = A @ z0 + B @ U[0]
    np.testing.assert_allclose(Z[1], z1, rtol=1e-14); np.testing.assert_allclose(Z[2], A @ z1 + B @ U[1], rtol=1e-13)
    Bb = rng.standard_normal((N, N * m))
    Z = rr.rollout_reference(A, Bb, z0, U, True, dtype=np.float64)
    z1 = A @ z0 + Bb @ np.kron(np.eye(m), z0[:, None]) @ U[0]
    np.testing.assert_allclose(Z[1], z1, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(Z[2], A @ z1 + Bb @ np.kron(np.eye(m), z1[:, None]) @ U[1], rtol=1e-12, atol=1e-13)
    assert np.array_equal(Z[0], z0)
