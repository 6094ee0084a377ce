"""Host-side check of the lift's plan and digit packing (csrc/kp_lift_plan.h), no device: tools/lift_plan_check.cpp is built with
the host compiler and run once per dictionary and batch size.

What is pinned:
  * the whole plan (nvars, nfull, fourier_degree, pure_fourier, points per workgroup, LDS bytes, stage_cols, refusal) against
    the restatement in tests/_lift_reference.py, for every case and row count of tests/test_gpu_lift_regimes.py (at the 256 compute
    units of an MI355X), and the regime each case is named for;
  * the threshold rows = 256 num_cu between 16 and 64 points per workgroup, from both sides, for 64, 256 and 304 compute units
    (and 256 for a device that reports none);
  * the 160 KB edges by their numbers: `linear, nzeta 10, poly 3` with a projection takes 64 points in 157 152 B with the
    descriptors staged, nzeta 11 falls to 16 points; the refusal of a projected 9-variable fourier dictionary;
  * the packed digits of every function of fourier degree 1 on 8 variables (all eight nibbles), degree 7 on 2 (radix 15, the
    largest that packs), degree 8 on 2 and degree 1 on 9 (both must be 0), against digits enumerated here with
    itertools.product, the last variable fastest;
  * a clean run of the program built with -fsanitize=address,undefined;
  * the long-double lift of tests/_lift_reference.py against oracle.koopman_oracle (written differently: kron and broadcasting
    against one column at a time) on every small case, to 1e-14 max(1, max|column|).
"""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _lift_reference as lr
from oracle import koopman_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MT = {"linear": 0, "bilinear": 1, "nonlinear": 2}
MI355X_CU = 256
REFUSAL = "kp_lift: dictionary too large for the LDS staging of the pcs projection"


def _build(tmp_path_factory, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lift_plan_tool") / "lift_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "koopman-realizations_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "lift_plan_check.cpp"), "-o", exe]
    return exe, subprocess.run(cmd + extra, capture_output=True, text=True)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe, r = _build(tmp_path_factory, [])
    assert r.returncode == 0, r.stderr
    return exe


def run_plan(exe, mt, nz, m, blocks, k, rows, num_cu, pads=False):
    out = subprocess.run([exe, str(MT[mt]), str(nz), str(m), str(k), str(rows), str(num_cu)] + (["pads"] if pads else [])
                         + [f"{kind}:{n}" for kind, n in blocks], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


@pytest.mark.parametrize("name", sorted(lr.CASES))
def test_plan_of_every_gpu_case_equals_the_restatement_and_the_regime_it_is_named_for(tool, name):
    c = lr.CASES[name]
    for spec in c.rows:
        rows = lr.row_count(spec, MI355X_CU)
        p = run_plan(tool, c.mt, c.nz, c.m, c.blocks, c.k, rows, MI355X_CU)
        assert p == lr.plan(c.mt, c.nz, c.m, c.blocks, c.k, rows, MI355X_CU)
        assert p["error"] is None and p["lt"] == c.lt and bool(p["stage_cols"] & 1) == c.staged
        assert tuple(lr.fourier_path(p, c.mt, c.blocks, c.k, w) for w in (lr.FULL, lr.ECON, lr.ROW)) == c.path


@pytest.mark.parametrize("num_cu", [64, 256, 304, 0])
@pytest.mark.parametrize("name", ["A-linear-poly2-at", "A-bilinear-poly3-pcs", "A-bilinear-fourier2", "A-linear11-poly3-pcs"])
def test_threshold_between_16_and_64_points_per_workgroup(tool, name, num_cu):
    c = lr.CASES[name]
    T = 256 * (num_cu or 256)
    below, at = (run_plan(tool, c.mt, c.nz, c.m, c.blocks, c.k, rows, num_cu) for rows in (T - 1, T))
    assert below == lr.plan(c.mt, c.nz, c.m, c.blocks, c.k, T - 1, num_cu) and at == lr.plan(c.mt, c.nz, c.m, c.blocks, c.k, T, num_cu)
    assert below["lt"] == 16 and at["lt"] == c.lt          # (nzeta 11 with a projection: 16 at any size)
    if c.lt == 64:
        assert at["lds"] > below["lds"] and at["stage_cols"] == below["stage_cols"]


def test_lds_edges_by_their_numbers(tool):
    n10, n11 = (lr.block_sizes(nz, ["poly"], [3]) for nz in (10, 11))
    assert n10 == [("poly", 275)] and n11 == [("poly", 352)]
    big = 256 * MI355X_CU + 37
    p = run_plan(tool, "linear", 10, 2, n10, 4, big, MI355X_CU)
    # per point: 10 variables + 2 inputs + 286 full functions = 298 doubles; 64 of them and 286 descriptors of 16 B
    assert (p["nfull"], p["lt"], p["lds"], p["stage_cols"], p["error"]) == (286, 64, 64 * 298 * 8 + 286 * 16, 1, None)
    assert p["lds"] == 157152 <= lr.LDS_BYTES and p == lr.plan("linear", 10, 2, n10, 4, big, MI355X_CU)
    p = run_plan(tool, "linear", 11, 2, n11, 4, big, MI355X_CU)
    assert 64 * 377 * 8 == 193024 > lr.LDS_BYTES
    assert (p["nfull"], p["lt"], p["lds"], p["stage_cols"], p["error"]) == (364, 16, 16 * 377 * 8 + 364 * 16, 1, None)
    assert p == lr.plan("linear", 11, 2, n11, 4, big, MI355X_CU)
    # descriptors that no longer fit beside 16 points: read from global memory, no fourier-only loop although nothing else is there
    p = run_plan(tool, "linear", 9, 1, [("fourier", 1)], 0, 17, MI355X_CU)
    assert (p["nfull"], p["lt"], p["lds"], p["stage_cols"], p["error"]) == (19692, 16, 16 * (9 + 1 + 27) * 8, 0, None)
    assert p["fourier_degree"] == 1 and not p["pure_fourier"] and p == lr.plan("linear", 9, 1, [("fourier", 1)], 0, 17, MI355X_CU)


@pytest.mark.parametrize("rows", [1, 17, 256 * MI355X_CU + 37])
def test_refusal_of_a_projection_too_wide_for_the_lds(tool, rows):
    p = run_plan(tool, "linear", 9, 1, [("fourier", 1)], 1, rows, MI355X_CU)
    assert p["error"] == REFUSAL and p["lt"] == 16 and p["lds"] == 16 * (9 + 1 + 27 + 19692) * 8 > lr.LDS_BYTES
    assert p == lr.plan("linear", 9, 1, [("fourier", 1)], 1, rows, MI355X_CU)


@pytest.mark.parametrize("degree,nvars,packs", [(1, 8, True), (7, 2, True), (8, 2, False), (1, 9, False)])
def test_packed_digits_of_every_fourier_function(tool, degree, nvars, packs):
    radix = 2 * degree + 1
    digits = list(itertools.product(range(radix), repeat=nvars))[1:]        # lexicographic: the last variable fastest; [0] is the constant
    assert len(digits) == radix ** nvars - 1
    expect = [sum(d << (4 * v) for v, d in enumerate(row)) if packs else 0 for row in digits]
    p = run_plan(tool, "linear", nvars, 1, [("fourier", degree)], 0, 17, MI355X_CU, pads=True)
    assert p["pads"] == expect == lr.fourier_pads(degree, nvars)
    assert p["fourier_degree"] == degree and p["pure_fourier"] == packs
    if packs:
        assert min(expect) > 0 and max(expect) < 2 ** 32            # no function but the constant has all digits zero
        assert max(row[0] for row in digits) == radix - 1 and max(e >> (4 * (nvars - 1)) for e in expect) == radix - 1
        # every digit reads back by shift and mask, also from the int32 the descriptor stores it in
        as_i32 = np.array(expect, dtype=np.uint32).view(np.int32)
        back = np.stack([(as_i32.view(np.uint32) >> (4 * v)) & 15 for v in range(8)], axis=1)
        assert np.array_equal(back[:, :nvars], np.array(digits)) and not back[:, nvars:].any()


def test_fourier_flags_of_mixed_dictionaries(tool):
    for blocks, fdeg, pure in [([("fourier", 1), ("fourier", 1)], 1, True), ([("fourier", 1), ("fourier", 2)], 0, False),
                               ([("poly", 3), ("fourier", 2)], 2, False), ([("fourier", 9)], 0, False), ([("fourier", 8)], 8, False),
                               ([("poly", 3)], 0, False), ([("poly", 0), ("fourier", 2)], 2, True), ([], 0, False)]:
        p = run_plan(tool, "linear", 2, 1, blocks, 0, 33, MI355X_CU)
        assert (p["fourier_degree"], p["pure_fourier"]) == (fdeg, pure), blocks
        assert p == lr.plan("linear", 2, 1, blocks, 0, 33, MI355X_CU)


def test_program_runs_clean_under_address_and_undefined_sanitizers(tmp_path_factory, tool):
    exe, r = _build(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler does not take -fsanitize=address,undefined: " + r.stderr[-200:])
    for name in ("A-linear10-poly3-pcs", "A-bilinear-fourier2", "B-fourier1-8vars", "B-fourier1-9vars", "B-fourier8-2vars", "C-five-bilinear-pcs"):
        c = lr.CASES[name]
        rows = lr.row_count(c.rows[-1], MI355X_CU)
        assert run_plan(exe, c.mt, c.nz, c.m, c.blocks, c.k, rows, MI355X_CU, pads=True) == run_plan(tool, c.mt, c.nz, c.m, c.blocks, c.k, rows, MI355X_CU, pads=True)
    assert run_plan(exe, "linear", 9, 1, [("fourier", 1)], 1, 17, MI355X_CU)["error"] == REFUSAL


@pytest.mark.parametrize("name", sorted(n for n in lr.CASES if not n.startswith("A-")))
def test_long_double_lift_agrees_with_the_oracle_on_the_small_cases(name):
    c = lr.CASES[name]
    dic = lr.case_dictionary(c)
    rows = lr.row_count(c.rows[-1], MI355X_CU)
    zeta, u = lr.case_points(c, rows)
    V = np.hstack([zeta, u]) if c.mt == "nonlinear" else zeta
    assert dic.basis.nfull == lr.plan(c.mt, c.nz, c.m, c.blocks, c.k, rows, MI355X_CU)["nfull"]
    for ref, got in [(lr.lift_full_ld(dic.basis, V), ko.lift_full(dic.basis, V)), (lr.econ_ld(dic, V), ko.econ_full(dic, V)),
                     (lr.rows_ld(dic, zeta, u), ko.lift_rows(dic, zeta, u))]:
        assert ref.dtype == np.longdouble and ref.shape == got.shape
        scale = np.maximum(1.0, np.abs(ref).max(axis=0))
        worst = (np.abs(got - ref) / scale).max()
        print(name, ref.shape, "oracle - long double, relative to max(1, |column|):", float(worst))
        assert worst <= 1e-14
