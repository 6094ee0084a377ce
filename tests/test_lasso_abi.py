"""kp_symm_product and timer slot 27 through the layers that need no GPU: declared in include/koopman_hip_lasso.h only,
exported by the built library, bound in _ffi.LASSO_SIGNATURES with one ctypes argument per declared parameter; the header's
constants equal _ffi's; the slot is documented where the others are; the shapes of tests/test_gpu_symm_product.py and
tests/test_gpu_lasso_regimes.py select the kernels those tests name."""
import ctypes as C
import os
import re

from koopman_realizations_amd import _ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def header():
    return open(os.path.join(INC, "koopman_hip_lasso.h")).read()


def declaration():
    m = re.search(r"^int\s+kp_symm_product\s*\(([^;]*)\)\s*;", header(), re.M)
    assert m, "kp_symm_product is not declared in koopman_hip_lasso.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_in_the_new_header_only():
    names = [a.split()[-1].lstrip("*") for a in declaration()]
    assert names == ["ctx", "G", "X", "W", "nc", "variant", "C", "ran"]
    for fn in os.listdir(INC):
        if fn != "koopman_hip_lasso.h":
            assert not re.search(r"\bkp_symm_product\s*\(", open(os.path.join(INC, fn)).read()), fn
    assert "kp_symm_product" not in F.SIGNATURES          # the MATLAB gateway covers koopman_hip.h one for one: no command for this


def test_exported_and_bound_with_the_declared_argument_types():
    assert hasattr(C.CDLL(F.LIB_PATH), "kp_symm_product")
    assert list(F.LASSO_SIGNATURES) == ["kp_symm_product"]
    res, argtypes = F.LASSO_SIGNATURES["kp_symm_product"]
    assert res is C.c_int

    def ctype(decl):
        if decl.startswith("kp_ctx*"):
            return F.vp
        if "double*" in decl:
            return F.c_dp
        if "int*" in decl:
            return F.c_ip
        assert decl.startswith("int "), decl
        return C.c_int
    assert argtypes == [ctype(a) for a in declaration()]
    assert getattr(F.lib(), "kp_symm_product").argtypes == argtypes


def test_constants_of_the_header_equal_those_of_the_binding():
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"^#define\s+(KP_[A-Z_0-9]+)\s+(0x[0-9a-fA-F]+u?|\d+)", header(), re.M)}
    assert F.TIMER_LASSO_KERNELS == 27
    assert {e: defs[f"KP_LASSO_RAN_EPT{e}"] for e in (4, 8, 16, 24, 0)} == F.LASSO_RAN_EPT
    assert defs["KP_LASSO_RAN_MULTI"] == F.LASSO_RAN_MULTI
    assert (defs["KP_LASSO_RAN_SMALL"], defs["KP_LASSO_RAN_TILED"], defs["KP_LASSO_RAN_NAIVE"]) == (F.LASSO_RAN_SMALL, F.LASSO_RAN_TILED, F.LASSO_RAN_NAIVE)
    assert {ra: defs["KP_LASSO_RAN_RA4"] << (ra - 4) for ra in range(4, 9)} == F.LASSO_RAN_RA
    assert {rb: defs[f"KP_LASSO_RAN_RB{rb}"] for rb in (2, 3, 4, 6)} == F.LASSO_RAN_RB
    assert (defs["KP_SYMM_BY_SHAPE"], defs["KP_SYMM_SMALL"], defs["KP_SYMM_TILED_RB"]) == (F.SYMM_BY_SHAPE, F.SYMM_SMALL, F.SYMM_TILED_RB)
    assert (defs["KP_SYMM_RAN_SMALL"], defs["KP_SYMM_RAN_NAIVE"], defs["KP_SYMM_RAN_TILED"]) == (F.SYMM_RAN_SMALL, F.SYMM_RAN_NAIVE, F.SYMM_RAN_TILED)
    bits = list(F.LASSO_RAN_EPT.values()) + [F.LASSO_RAN_MULTI, F.LASSO_RAN_SMALL, F.LASSO_RAN_TILED, F.LASSO_RAN_NAIVE] \
        + list(F.LASSO_RAN_RA.values()) + list(F.LASSO_RAN_RB.values())
    assert sorted(bits) == [1 << k for k in range(18)]          # one bit each, none shared


def test_timer_slot_is_documented_where_the_others_are():
    text = open(os.path.join(INC, "koopman_hip.h")).read()
    block = text[:text.index("int kp_timer_get")]
    assert re.search(r"\b27: not a time - a bit mask of the\s+\* kernels", block) and "KP_LASSO_RAN_" in block
    src = open(os.path.join(ROOT, "koopman-realizations_amd", "csrc", "kp_context.hip")).read()
    assert "which >= 28" in src


def test_shapes_of_the_gpu_tests_select_the_kernels_they_name():
    from test_gpu_symm_product import TILED_W, pick_ra
    from test_gpu_lasso_regimes import EPT_SHAPES, expected_ept
    for W, (ra, nkb) in TILED_W.items():
        assert pick_ra(W) == ra and -(-W // 16) == nkb, W
    assert {ra for ra, _ in TILED_W.values()} == {4, 5, 6, 7, 8}
    assert -(-130 // (16 * 5)) == 2 and 130 - 80 == 50          # two row tiles, the second with 50 of 80 rows
    assert pick_ra(336) == 7
    for cus in (32, 64, 256, 304):                              # wpv = 32 on any device with at least 32 CUs
        assert [expected_ept(32 * nc, 1, cus) for nc, _ in EPT_SHAPES] == [e for _, e in EPT_SHAPES]
    assert [e for _, e in EPT_SHAPES] == [4, 8, 8, 16, 16, 24, 24, 0]
