"""GPU tests of kp_sweep_eval_nested / kp_sweep_eval (csrc/kp_sweep.hip, kp_sweep_gram.hip) in every kernel the dictionary can select, beyond the
1-state / 1-input shapes of the benchmark.  Reference: tests/_sweep_reference.py (the oracle for full exponent tables, its
plain numpy restatement for sparse ones, a long-double rollout of the device's own model).  Every case proves which kernels
it ran through kp_timer_get(14) = 1000 G + 100 F + 10 U + R (include/koopman_hip.h).

Cases (3 systems - no multiple of 4: a rollout4 wave holds jobs of two degrees -, 3 trials of 60 rows = 176 pairs: one full
128-pair tile and a ragged one, 40 validation rows); n, m, monomials beyond the variables -> code:
  A  linear    2,2  full degree 3 (W 12)            4201  mfma run-time F=2, rollout4, projection m=2
  B  linear    3,3  xy, yz, xyz (W 10)              4301  mfma F=3, rollout4 n=3, m=3
  C  linear    4,1  x1^2, x1x2x3x4 (W 8)            4401  mfma F=4, rollout4 n=4
  D  bilinear  2,1  full degree 2 (W 12)            4211  mfma UPRO F=2
  E1 bilinear  3,2  xyz (N 5, W 15)                 4311  mfma UPRO F=3
  E2 bilinear  3,3  none (N 4, W 16)                4111  mfma UPRO F=1, m=3, the full 16-wide tile
  F  bilinear  4,1  x1x2x3x4 (W 12)                 4411  mfma UPRO F=4
  G  bilinear  1,1  x^9 (W 6)                       4201  table too large for UPRO: the input is a second factor
  H  bilinear  4,1  x1^2, x1x2x3x4 (W 14)           4501  no UPRO, F=5
  I  nonlinear 2,2  full degree 2 on [zeta; u] (15) 4201  mfma F=2 on 4 variables, rollout4 with two inputs
  J  nonlinear 2,3  none (5 variables)              1001  kp_traj_gram_kernel, rollout4 with three inputs
  K  nonlinear 4,1  none                            1001  kp_traj_gram_kernel, rollout4 n=4
  L  linear    5,1  none (W 7)                      1002  kp_traj_gram_kernel, kp_sweep_rollout_nested_kernel
  M  bilinear  7,1  none (W 16)                     1002  the same, bilinear, full tile
  N  nonlinear 5,3  none (8 variables: the limit)   1002  the same, nonlinear
  O  linear    1,1  x^13                            3101  mfma<1,13,1,false>  } the compile-time shapes, which the cols
  P  bilinear  1,1  x^6                             3111  mfma<1,6,1,true>    } kernels shadow for the canonical
  Q  nonlinear 1,1  x^4, x^3 u                      3201  mfma<2,4,2,false>   } dictionaries
  R  bilinear  1,1  none                            4111  mfma UPRO F=1 with a run-time shape
The issue's case E (bilinear, n = m = 3, xyz, "N = 4, W = 16") does not exist: with xyz N = 5 and W = 20 > 16.  A three-factor
monomial needs n >= 3, so N >= 5 and W = 5 (m + 1) <= 16 forces m <= 2: UPRO F=3 with m = 3 is unreachable under W <= 16.  E1
covers UPRO F=3 (m = 2, W = 15), E2 covers m = 3 on the full 16-wide tile (UPRO F=1).  Every other regime of the list is hit.

Checks per case, over all systems, degrees and error components:
  (a) status 0 everywhere, timer 14 = the code above;
  (b) K of every degree within 1e-9 max|K_ref| of the reference least squares;
  (c) err within 1e-4 max(1, |w|) of the whole reference pipeline;
  (d) err within 4 * 16 * Tv * 2.2e-16 of the long-double rollout of the device's OWN K (bilinear, nonlinear), or within
      max(1e-9, 50 cond(L)^2 2.2e-16) of the long-double rollout of the reference projection of the device's K (linear);
  (e) a second call bitwise equal; system 1 alone bitwise what it was as the middle one of three;
  (f) kp_sweep_eval on the top-degree dictionary: K within 1e-8 max|K_ref|, err within 1e-7 max(1, |w|) of the nested top
      degree, timer 14 = 5003.
Largest observed ratio difference / tolerance per case on the MI355X, (b) | (c) | (d):
  A 1.4e-4 | 7.5e-11 | 6.4e-6    B 7.2e-6 | 3.7e-11 | 3.2e-6    C 8.1e-6 | 7.6e-11 | 5.8e-6    D 5.9e-5 | 9.9e-11 | 2.1e-4
  E1 6.3e-6 | 2.0e-10 | 4.6e-4   E2 5.3e-6 | 7.2e-11 | 3.1e-4   F 2.6e-5 | 9.9e-11 | 2.0e-4    G 3.9e-6 | 9.6e-11 | 2.8e-4
  H 9.4e-5 | 7.6e-11 | 5.2e-4    I 7.7e-6 | 3.3e-11 | 2.3e-4    J 5.1e-6 | 2.2e-11 | 2.3e-4    K 5.0e-6 | 5.0e-11 | 1.9e-4
  L 5.0e-6 | 2.1e-11 | 2.6e-6    M 1.5e-5 | 5.7e-11 | 1.9e-4    N 2.7e-6 | 3.0e-11 | 3.7e-4    O 4.4e-6 | 9.8e-12 | 1.3e-6
  P 6.6e-6 | 8.6e-11 | 1.2e-4    Q 1.6e-6 | 2.0e-11 | 1.6e-4    R 1.1e-6 | 4.9e-11 | 2.0e-4    lasso (d) 7.9e-4
  fallback kernels (KP_SWEEP_GRAM_OLD, KP_SWEEP_NO_ROLLOUT4): A 1.6e-4 | 6.9e-11 | 2.6e-6, D 3.1e-5 | 1.0e-10 | 2.8e-4,
  I 5.6e-6 | 3.3e-11 | 2.3e-4, G 3.6e-6 | 5.3e-11 | 3.0e-4.  No (d) ratio comes near 0.1.
Found by cases G, O, P, Q (before the fix K of the top degree was off by 100 %, ratio 1.7e9 in G): the nested sweep accumulated
its Grams in a Chebyshev internal basis for EVERY table, but [T_1, T_9, 1] does not span [x, x^9, 1] - only tables that hold,
with a monomial, every term of its Chebyshev expansion (the full tables of def_polyLift; x1^2 with the constant) are served
by it.  kp_sweep_eval_nested now keeps the monomials as the internal basis of any other table.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import sweep
from koopman_realizations_amd.device import Basis, Traj
from oracle import koopman_oracle as ko
import _sweep_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [c for c in sr.CASES if c != "LASSO"]


def _basis(ctx, name):
    mt, n, m, nv, ex, D, N, W, code = sr.case_dims(name)
    b = Basis(ctx, mt, n, m, [("poly", ex.astype(np.uint8))], None)
    assert (b.N, b.W) == (N, W)
    return b


def _nested(ctx, name, systems, lasso=np.inf):
    """One kp_sweep_eval_nested call on `systems`: err (D, nb, n), status (D, nb), K per degree, timer 14."""
    mt, n, m, nv, ex, D, N, W, code = sr.case_dims(name)
    traj = Traj(ctx, *sweep._stack_raw(list(systems)))
    basis = _basis(ctx, name)
    try:
        err, st = traj.sweep_eval_nested(basis, D, lasso)
        t14 = int(ctx.timer(14))
        Ks = []
        for dj in range(D):
            Nj = nv + sr.rows_of_degree(ex, dj + 1).shape[0] + 1
            Ks.append(np.array(traj.nested_K(dj, sr.width(mt, m, Nj))))
    finally:
        basis.close(); traj.close()
    return err, st, Ks, t14


def _flat(ctx, name, systems, lasso=np.inf):
    traj = Traj(ctx, *sweep._stack_raw(list(systems)))
    basis = _basis(ctx, name)
    try:
        err, K, st = traj.sweep_eval(basis, lasso, want_K=True)
        t14 = int(ctx.timer(14))
    finally:
        basis.close(); traj.close()
    return err, np.array(K), st, t14


def _check_K(name, Ks, ref, tol=1e-9):
    """(b).  Returns the largest difference / tolerance."""
    worst = 0.0
    for dj, Kd in enumerate(Ks):
        for i in range(Kd.shape[0]):
            Kref = ref[dj][i]["K"]
            ratio = np.abs(Kd[i] - Kref).max() / (tol * np.abs(Kref).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, "K", dj, i, ratio)
    return worst


def _check_err(name, err, ref):
    """(c).  Returns the largest difference / tolerance."""
    worst = 0.0
    for dj in range(err.shape[0]):
        for i in range(err.shape[1]):
            w = ref[dj][i]["err"]
            ratio = (np.abs(err[dj, i] - w) / (1e-4 * np.maximum(1.0, np.abs(w)))).max()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, "err", dj, i, err[dj, i], w)
    return worst


def _check_rollout(name, err, Ks, ref, systems):
    """(d).  Returns the largest difference / tolerance."""
    mt, n, m = sr.CASES[name][:3]
    worst = 0.0
    for i, s in enumerate(systems):
        pairs, val = sr.prepare(s)
        for dj in range(err.shape[0]):
            r = ref[dj][i]
            w = sr.rollout_reference_ld(mt, n, m, r["ex"], Ks[dj][i], pairs, val)
            tol = sr.linear_rollout_tol(r["condL"]) if mt == "linear" else sr.rollout_floor(val["y"].shape[0])
            ratio = (np.abs(err[dj, i] - w) / (tol * np.maximum(1.0, np.abs(w)))).max()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, "rollout", dj, i, err[dj, i], w, ratio)
    return worst


def run_case(ctx, name, code=None, flat=True, determinism=True):
    """Checks (a)-(f) of one case; returns the ratios of (b), (c), (d).  (Also what the child process of the environment
    switches runs, with the code of the fallback kernels.)"""
    mt, n, m, nv, ex, D, N, W, want_code = sr.case_dims(name)
    systems, ref = sr.case_systems(name), sr.case_reference(name)
    err, st, Ks, t14 = _nested(ctx, name, systems)
    assert (st == 0).all(), (name, st)                                                     # (a)
    assert t14 == (want_code if code is None else code), (name, t14)
    rb = _check_K(name, Ks, ref)                                                           # (b)
    rc = _check_err(name, err, ref)                                                        # (c)
    rd = _check_rollout(name, err, Ks, ref, systems)                                       # (d)
    print("RATIOS %-5s code %d  (b) %.3g  (c) %.3g  (d) %.3g" % (name, t14, rb, rc, rd))
    if determinism:                                                                        # (e)
        err2, st2, Ks2, _ = _nested(ctx, name, systems)
        assert np.array_equal(err, err2) and np.array_equal(st, st2) and all(np.array_equal(a, b) for a, b in zip(Ks, Ks2)), name
        err1, st1, Ks1, _ = _nested(ctx, name, systems[1:2])
        assert (st1 == 0).all() and np.array_equal(err1[:, 0], err[:, 1]), (name, err1[:, 0] - err[:, 1])
        assert all(np.array_equal(a[0], b[1]) for a, b in zip(Ks1, Ks)), name
    if flat:                                                                               # (f)
        errf, Kf, stf, t14f = _flat(ctx, name, systems)
        assert (stf == 0).all() and t14f == sr.FLAT_CODE, (name, stf, t14f)
        for i in range(len(systems)):
            Kref = ref[D - 1][i]["K"]
            assert np.abs(Kf[i] - Kref).max() <= 1e-8 * np.abs(Kref).max(), (name, "flat K", i, np.abs(Kf[i] - Kref).max() / np.abs(Kref).max())
        w = err[D - 1]
        assert (np.abs(errf - w) <= 1e-7 * np.maximum(1.0, np.abs(w))).all(), (name, "flat err", errf, w)
    return rb, rc, rd


@pytest.mark.parametrize("name", TABLE)
def test_sweep_case_against_the_reference(ctx, name):
    run_case(ctx, name)


def test_the_cases_cover_every_regime_of_the_dispatch():
    """What the per-case timer-14 assertions add up to: G = 1, 3, 4 (2 is the canonical 1-D dictionaries of test_gpu_sweep.py),
    F = 1 .. 5, U = 0 and 1 - with F = 2, 3, 4 -, R = 1 and 2 nested and 3 flat, G = 5 flat."""
    codes = {sr.case_dims(c)[8] for c in TABLE}
    assert {c // 1000 for c in codes} == {1, 3, 4}
    assert {(c // 100) % 10 for c in codes if c // 1000 in (3, 4)} == {1, 2, 3, 4, 5}
    assert {(c // 100) % 10 for c in codes if (c // 10) % 10 == 1} == {1, 2, 3, 4}
    assert {(c // 100) % 10 for c in codes if (c // 10) % 10 == 0 and c // 1000 == 4} == {2, 3, 4, 5}
    assert {c % 10 for c in codes} == {1, 2} and sr.FLAT_CODE // 1000 == 5 and sr.FLAT_CODE % 10 == 3
    assert {c for c in codes if c // 1000 == 3} == {3101, 3111, 3201}


# ---- edges: pair counts around the 128-pair tile and the mfma kernel's four-tile prefetch (K and status only) ----
@pytest.mark.parametrize("name", ["A", "L"])
@pytest.mark.parametrize("k,T,npairs", [(1, 50, 48), (1, 130, 128), (2, 66, 129), (2, 258, 513)])
def test_pair_counts_at_the_tile_edges(ctx, name, k, T, npairs):
    assert k * (T - 1) - 1 == npairs
    systems, ref = sr.case_systems(name, k, T), sr.case_reference(name, k, T)
    assert sr.prepare(systems[0])[0]["alpha"].shape[0] == npairs
    err, st, Ks, t14 = _nested(ctx, name, systems)
    assert (st == 0).all() and t14 == sr.case_dims(name)[8] and np.isfinite(err).all()
    _check_K(name, Ks, ref)


@pytest.mark.parametrize("name", ["D", "M"])
def test_validation_trial_of_one_step(ctx, name):
    """Tv = 2: a single simulated step."""
    systems, ref = sr.case_systems(name, sr.K_TRIALS, sr.T_TRAIN, 2), sr.case_reference(name, sr.K_TRIALS, sr.T_TRAIN, 2)
    err, st, Ks, t14 = _nested(ctx, name, systems)
    assert (st == 0).all() and t14 == sr.case_dims(name)[8]
    _check_K(name, Ks, ref)
    _check_err(name, err, ref)
    _check_rollout(name, err, Ks, ref, systems)


def test_validation_trial_without_a_step_is_refused(ctx):
    """Tv = 1: the oracle's val_model takes it (sim = real, error 0), kp_traj_upload does not (Tv >= 2): a clean error."""
    systems, ref = sr.case_systems("D", sr.K_TRIALS, sr.T_TRAIN, 1), sr.case_reference("D", sr.K_TRIALS, sr.T_TRAIN, 1)
    assert all((r["err"] == 0.0).all() for row in ref for r in row)
    with pytest.raises(kra.KoopmanHipError):
        Traj(ctx, *sweep._stack_raw(list(systems)))


@pytest.mark.parametrize("name", ["D", "M"])
def test_a_zero_system_between_two_others(ctx, name):
    """All outputs and inputs of the middle system are zero: its status is set and its n error components are NaN at every
    degree, and both neighbours are bitwise what they are with an ordinary system in its place."""
    systems = list(sr.case_systems(name))
    err, st, Ks, _ = _nested(ctx, name, systems)
    systems[1] = sr.zero_system(systems[1])
    errz, stz, Ksz, t14 = _nested(ctx, name, systems)
    assert t14 == sr.case_dims(name)[8]
    assert (stz[:, 1] != 0).all() and np.isnan(errz[:, 1, :]).all()
    for i in (0, 2):
        assert (stz[:, i] == 0).all() and np.array_equal(errz[:, i], err[:, i])
        assert all(np.array_equal(a[i], b[i]) for a, b in zip(Ksz, Ks))


# ---- the lasso re-solve of flagged systems, in both calls ----
def test_lasso_branch_of_both_sweep_calls(ctx):
    """Nonlinear, n = 2, m = 1, full degree 2 (W = 10); lasso such that t = lasso N is half of |K_LS|_1 of system 0 at the top
    degree.  A (system, degree) whose |K_LS|_1 exceeds t_j = lasso N_j is re-solved: the bounds of
    test_lasso_active_constraint_matches_oracle (the same solver); one that does not keeps its least-squares K (b).  err by (d)
    on the device's K either way."""
    name = "LASSO"
    mt, n, m, nv, ex, D, N, W, code = sr.case_dims(name)
    systems, ref = sr.case_systems(name), sr.case_reference(name)
    lasso = 0.5 * np.abs(ref[D - 1][0]["K"]).sum() / N
    err, st, Ks, t14 = _nested(ctx, name, systems, lasso)
    assert (st == 0).all() and t14 == code
    errf, Kf, stf, t14f = _flat(ctx, name, systems, lasso)
    assert (stf == 0).all() and t14f == sr.FLAT_CODE
    n_active = 0
    for dj in range(D):
        Nj = nv + sr.rows_of_degree(ex, dj + 1).shape[0] + 1
        t = lasso * Nj
        for i in range(len(systems)):
            r = ref[dj][i]
            l1 = np.abs(r["K"]).sum()
            assert abs(l1 - t) > 1e-3 * t                             # no (system, degree) sits on the edge of the flag
            got = [Ks[dj][i]] + ([Kf[i]] if dj == D - 1 else [])
            for K in got:
                if l1 > t:
                    Ko = ko.koopman_lasso(r["G"], r["C"], t)
                    assert abs(np.abs(K).sum() - t) < 1e-8 * t, (dj, i, np.abs(K).sum() / t)
                    assert ko.lasso_kkt_residual(r["G"], r["C"], K, t) < 1e-6 * np.abs(r["C"]).max(), (dj, i)
                    assert np.abs(K - Ko).max() < 1e-6 * np.abs(Ko).max(), (dj, i, np.abs(K - Ko).max() / np.abs(Ko).max())
                else:
                    assert np.abs(K - r["K"]).max() <= 1e-9 * np.abs(r["K"]).max(), (dj, i)
            n_active += l1 > t
    assert n_active >= 1
    rd = _check_rollout(name, err, Ks, ref, systems)
    pairs_val = [sr.prepare(s) for s in systems]
    for i, (pairs, val) in enumerate(pairs_val):                      # flat: the rollout of its own K
        w = sr.rollout_reference_ld(mt, n, m, ex, Kf[i], pairs, val)
        assert (np.abs(errf[i] - w) <= sr.rollout_floor(val["y"].shape[0]) * np.maximum(1.0, np.abs(w))).all(), (i, errf[i], w)
    print("RATIOS LASSO code %d  (d) %.3g  active %d" % (t14, rd, n_active))
    # a finite lasso that flags nothing: every degree keeps its least-squares K
    hi = 1.5 * max(np.abs(r["K"]).sum() / (nv + r["ex"].shape[0] + 1) for row in ref for r in row)
    assert hi < 1e6
    err_hi, st_hi, Ks_hi, _ = _nested(ctx, name, systems, hi)
    assert (st_hi == 0).all()
    _check_K(name, Ks_hi, ref)
    _check_err(name, err_hi, ref)


# ---- the fallback kernels behind the environment switches, at shapes the default kernels also serve ----
_CHILD = """
import sys, faulthandler
faulthandler.enable()
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import koopman_realizations_amd as kra
import test_gpu_sweep_shapes as t
ctx = kra.Context(0)
for name in ("A", "D", "I", "G"):
    t.run_case(ctx, name, code=1002, flat=False, determinism=False)
ctx.close()
print("CHILD_OK")
"""


def test_fallback_kernels_behind_the_environment_switches():
    """KP_SWEEP_GRAM_OLD=1 KP_SWEEP_NO_ROLLOUT4=1 (read once per process, hence a fresh child): cases A, D and I through
    kp_traj_gram_kernel and kp_sweep_rollout_nested_kernel - timer 14 = 1002 - with (b), (c) and (d) as above; and G, the sparse
    table that kp_traj_gram_kernel, too, has to accumulate in monomials."""
    env = dict(os.environ, KP_SWEEP_GRAM_OLD="1", KP_SWEEP_NO_ROLLOUT4="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=240, env=env)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.count("code 1002") == 4
