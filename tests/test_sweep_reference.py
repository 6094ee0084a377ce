"""CPU checks of tests/_sweep_reference.py, the reference that tests/test_gpu_sweep_shapes.py holds the sweep kernels against:
its plain restatement equals oracle/koopman_oracle.py wherever the oracle applies (full tables), and the inputs of every GPU
case are benign enough that a float64 and a long-double rollout of the same model agree within the rollout tolerance the
GPU test uses - so that tolerance measures the kernel, not the system."""
import numpy as np
import pytest

import _sweep_reference as sr
from oracle import koopman_oracle as ko

FULL = [name for name in sr.CASES if sr.is_full(sr.case_dims(name)[4], sr.case_dims(name)[3], sr.case_dims(name)[5])]


def test_the_case_table_has_the_widths_the_kernels_admit():
    for name in sr.CASES:
        mt, n, m, nv, ex, D, N, W, code = sr.case_dims(name)
        assert W <= 16 and m <= 3 and nv <= 8, name
        deg = ex.sum(axis=1)
        assert (np.diff(deg) >= 0).all() and (deg >= 2).all(), name            # ordered by total degree, no repeat of a variable
    assert {n_: sr.case_dims(n_)[7] for n_ in ("A", "D", "E1", "E2", "I", "M")} == {"A": 12, "D": 12, "E1": 15, "E2": 16, "I": 15, "M": 16}
    assert set(FULL) >= {"A", "D", "I", "LASSO"}


@pytest.mark.parametrize("name", FULL)
def test_sparse_restatement_equals_the_oracle_on_full_tables(name):
    mt, n, m, nv, ex, D, N, W, code = sr.case_dims(name)
    for s in sr.case_systems(name):
        pairs, val = sr.prepare(s)
        for j in range(1, D + 1):
            exj = sr.rows_of_degree(ex, j)
            assert (exj == ko.poly_exponents(nv, j)[nv:]).all()
            a = sr.sparse_pipeline(mt, n, m, exj, pairs, val)
            b = sr.oracle_pipeline(mt, n, m, j, pairs, val)
            # two lstsq calls on identically valued matrices, columns formed by repeated multiplication against `**`
            assert np.abs(a["K"] - b["K"]).max() <= 1e-12 * np.abs(b["K"]).max(), (name, j)
            assert np.abs(a["err"] - b["err"]).max() <= 1e-12, (name, j)
            assert np.abs(a["G"] - b["G"]).max() <= 1e-13 * np.abs(b["G"]).max()
            if mt == "linear":
                assert abs(a["condL"] - b["condL"]) <= 1e-9 * b["condL"]


@pytest.mark.parametrize("name", list(sr.CASES))
def test_float64_and_long_double_rollouts_agree_within_the_rollout_floor(name):
    """A condition on the inputs: where it fails, the system amplifies rounding and has to change - not the floor."""
    mt, n, m, nv, ex, D, N, W, code = sr.case_dims(name)
    ref = sr.case_reference(name)
    for dj in range(D):
        for i, s in enumerate(sr.case_systems(name)):
            r = ref[dj][i]
            pairs, val = sr.prepare(s)
            assert np.isfinite(r["err"]).all() and (r["err"] < 1.0).all(), (name, dj, i, r["err"])
            ld = sr.rollout_reference_ld(mt, n, m, r["ex"], r["K"], pairs, val)
            tol = sr.linear_rollout_tol(r["condL"]) if mt == "linear" else sr.rollout_floor(val["y"].shape[0])
            assert np.abs(ld - r["err"]).max() <= tol, (name, dj, i, np.abs(ld - r["err"]).max() / tol)
            if mt != "linear":                                       # also a tenth of it: room for the kernel's own rounding
                assert np.abs(ld - r["err"]).max() <= 0.1 * tol, (name, dj, i, np.abs(ld - r["err"]).max() / tol)
            assert np.linalg.cond(sr.px_py(mt, r["ex"], pairs)[0]) <= 1e4, (name, dj, i)      # (b) leaves decades of room


def test_long_double_is_wider_than_float64_here():
    assert np.finfo(np.longdouble).eps < 1e-18
