"""kp_eig through the layers that need no GPU: declared in include/koopman_hip_spectrum.h only, exported by the built library,
bound in _ffi.SPECTRUM_SIGNATURES with one ctypes argument per declared parameter; the header's constants equal _ffi's."""
import ctypes as C
import os
import re

from koopman_realizations_amd import _ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def header():
    return open(os.path.join(INC, "koopman_hip_spectrum.h")).read()


def declaration():
    m = re.search(r"^int\s+kp_eig\s*\(([^;]*)\)\s*;", header(), re.M)
    assert m, "kp_eig is not declared in koopman_hip_spectrum.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_in_the_new_header_only():
    names = [a.split()[-1].lstrip("*") for a in declaration()]
    assert names == ["ctx", "nb", "n", "A", "want_vectors", "wr", "wi", "V", "iters", "status"]
    for fn in os.listdir(INC):
        if fn != "koopman_hip_spectrum.h":
            assert not re.search(r"\bkp_eig\s*\(", open(os.path.join(INC, fn)).read()), fn
    assert "kp_eig" not in F.SIGNATURES          # the MATLAB gateway covers koopman_hip.h one for one: no command for this


def test_exported_by_the_library():
    assert hasattr(C.CDLL(F.LIB_PATH), "kp_eig")


def test_bound_with_the_declared_argument_types():
    assert list(F.SPECTRUM_SIGNATURES) == ["kp_eig"]
    res, argtypes = F.SPECTRUM_SIGNATURES["kp_eig"]
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
    assert getattr(F.lib(), "kp_eig").argtypes == argtypes


def test_constants_of_the_header_equal_those_of_the_binding():
    defs = dict(re.findall(r"^#define\s+(KP_EIG_[A-Z_]+)\s+(\d+)", header(), re.M))
    assert int(defs["KP_EIG_MAXN"]) == F.EIG_MAXN == 512
    assert int(defs["KP_EIG_WAVE_MAX"]) == F.EIG_WAVE_MAX == 32
    assert int(defs["KP_EIG_LDS_MAXN_VEC"]) == F.EIG_LDS_MAXN_VEC
    assert int(defs["KP_EIG_LDS_MAXN_VAL"]) == F.EIG_LDS_MAXN_VAL
    assert (F.TIMER_EIG, F.TIMER_EIG_REGIME) == (22, 23)
    # the header's formula: nmat n (n + 1) + 4 n + 64 doubles within 160 KB
    fits = lambda n, nmat: nmat * n * (n + 1) + 4 * n + 64 <= 160 * 1024 // 8
    assert fits(F.EIG_LDS_MAXN_VEC, 2) and not fits(F.EIG_LDS_MAXN_VEC + 1, 2)
    assert fits(F.EIG_LDS_MAXN_VAL, 1) and not fits(F.EIG_LDS_MAXN_VAL + 1, 1)


def test_timer_slots_are_documented_where_the_others_are():
    text = open(os.path.join(INC, "koopman_hip.h")).read()
    block = text[:text.index("int kp_timer_get")]
    assert re.search(r"\b22: the kernel of the most recent batched eigensolver", block) and "23: not" in block
    assert "KP_EIG_REGIME" in block
