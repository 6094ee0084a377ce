"""kp_tn_product through the layers that need no GPU: declared in include/koopman_hip_tn.h only, exported by the built library,
bound in _ffi.TN_SIGNATURES with one ctypes argument per declared parameter and absent from _ffi.SIGNATURES; the header's
constants equal _ffi's; the restatements of the launcher's split count and staging choice in tests/test_gpu_tn_product.py give
what that test's case tables name."""
import ctypes as C
import os
import re

from koopman_realizations_amd import _ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def header():
    return open(os.path.join(INC, "koopman_hip_tn.h")).read()


def declaration():
    m = re.search(r"^int\s+kp_tn_product\s*\(([^;]*)\)\s*;", header(), re.M)
    assert m, "kp_tn_product is not declared in koopman_hip_tn.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_in_the_new_header_only():
    names = [a.split()[-1].lstrip("*") for a in declaration()]
    assert names == ["ctx", "A", "lda", "B", "ldb", "M", "N", "K", "C", "ldc", "alpha", "beta", "tri", "nsplit", "wa", "wb", "form", "flags", "ran"]
    for fn in os.listdir(INC):
        if fn != "koopman_hip_tn.h":
            assert not re.search(r"\bkp_tn_product\s*\(", open(os.path.join(INC, fn)).read()), fn
    assert "kp_tn_product" not in F.SIGNATURES            # the MATLAB gateway covers koopman_hip.h one for one: no command for this


def test_exported_and_bound_with_the_declared_argument_types():
    assert hasattr(C.CDLL(F.LIB_PATH), "kp_tn_product")
    assert list(F.TN_SIGNATURES) == ["kp_tn_product"]
    res, argtypes = F.TN_SIGNATURES["kp_tn_product"]
    assert res is C.c_int

    def ctype(decl):
        if decl.startswith("kp_ctx*"):
            return F.vp
        if "double*" in decl:
            return F.c_dp
        if "int*" in decl:
            return F.c_ip
        if decl.startswith("int64_t "):
            return C.c_int64
        if decl.startswith("double "):
            return C.c_double
        assert decl.startswith("int "), decl
        return C.c_int
    assert argtypes == [ctype(a) for a in declaration()]
    assert getattr(F.lib(), "kp_tn_product").argtypes == argtypes


def test_constants_of_the_header_equal_those_of_the_binding():
    defs = {k: int(v, 0) for k, v in re.findall(r"^#define\s+(KP_TN_[A-Z_0-9]+)\s+(0x[0-9a-fA-F]+|\d+)", header(), re.M)}
    flags = (defs["KP_TN_MISALIGN"], defs["KP_TN_SAME"], defs["KP_TN_MIRROR"])
    assert flags == (F.TN_MISALIGN, F.TN_SAME, F.TN_MIRROR)
    assert sorted(flags) == [1, 2, 4]                          # one bit each, none shared
    assert (defs["KP_TN_RAN_FORM"], defs["KP_TN_RAN_VEC"], defs["KP_TN_FORM_SMALL"]) == (F.TN_RAN_FORM, F.TN_RAN_VEC, F.TN_FORM_SMALL)
    assert sorted(defs) == ["KP_TN_FORM_SMALL", "KP_TN_MIRROR", "KP_TN_MISALIGN", "KP_TN_RAN_FORM", "KP_TN_RAN_VEC", "KP_TN_SAME"]
    # the forms the binding names are those of tng_shapes(), in its order
    src = open(os.path.join(ROOT, "koopman-realizations_amd", "csrc", "kp_tn_gemm.h")).read()
    m = re.search(r"sh\[TNG_NSHAPES\]\s*=\s*\{(.*)\};", src)
    assert tuple((int(a), int(b)) for a, b in re.findall(r"\{(\d+),\s*(\d+),", m.group(1))) == F.TN_SHAPES
    assert re.search(r"#define\s+TNG_NSHAPES\s+4\b", src) and len(F.TN_SHAPES) == F.TN_FORM_SMALL == 4


def test_restated_formulas_give_what_the_gpu_tests_case_tables_name():
    from test_gpu_tn_product import SPLITS, STAGING, expected_vec, splits_that_run
    assert splits_that_run(40, 5) == 3 and 40 - 2 * 16 == 8    # five asked for, three run, the last with 8 indices
    assert splits_that_run(257, 5) == 5 and 257 - 4 * 64 == 1
    assert splits_that_run(100, 3) == 3 and -(-(-(-100 // 3)) // 16) * 16 == 48          # k_lo = 48, 96: whole blocks beyond the first split
    for (K, ns), want in SPLITS.items():
        assert splits_that_run(K, ns) == want, (K, ns)
    assert {K for K, _ in SPLITS} == {40, 100, 257} and {ns for _, ns in SPLITS} == {2, 3, 5}
    assert all(splits_that_run(K, 1) == 1 for K in (1, 16, 1000)) and splits_that_run(15, 2) == 1
    for (pad, mis), vecs in STAGING.items():
        for K in (1, 15, 16, 17, 31, 32, 33, 48):
            for code in (0, 1, 3, 4):
                assert expected_vec(code, K + pad, K + pad, mis) == vecs[K % 2], (K, pad, mis, code)
            assert expected_vec(2, K + pad, K + pad, mis) == 0
    assert {pad for pad, _ in STAGING} >= {0, 6}               # ld == K and ld == K + 6 at every K
    assert expected_vec(0, 34, 35, False) == 0 and expected_vec(0, 35, 34, False) == 0 and expected_vec(3, 34, 34, False) == 1
