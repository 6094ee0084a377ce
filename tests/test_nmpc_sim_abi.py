"""kp_nmpc_simulate through the layers that need no GPU: declared in include/koopman_hip_nmpc.h, exported by the built
library, bound in _ffi.NMPC_SIGNATURES with the declaration's argument list."""
import ctypes as C
import os
import re

from koopman_realizations_amd import _ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declaration():
    text = open(os.path.join(ROOT, "include", "koopman_hip_nmpc.h")).read()
    m = re.search(r"^int\s+kp_nmpc_simulate\s*\(([^;]*)\)\s*;", text, re.M)
    assert m, "kp_nmpc_simulate is not declared in koopman_hip_nmpc.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_in_the_header():
    args = declaration()
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["nmpc", "nb", "nref", "ref", "ref_shared", "y0", "u0", "warm", "U", "Y", "info", "steps_done", "status"]


def test_exported_by_the_library():
    lib = C.CDLL(F.LIB_PATH)
    assert hasattr(lib, "kp_nmpc_simulate")


def test_bound_with_the_declared_argument_types():
    assert "kp_nmpc_simulate" in F.NMPC_SIGNATURES
    res, argtypes = F.NMPC_SIGNATURES["kp_nmpc_simulate"]
    assert res is C.c_int

    def ctype(decl):
        if decl.startswith("kp_nmpc*"):
            return F.vp
        if "double*" in decl:
            return F.c_dp
        if "int*" in decl:
            return F.c_ip
        assert decl.startswith("int "), decl
        return C.c_int
    assert argtypes == [ctype(a) for a in declaration()]
    assert getattr(F.lib(), "kp_nmpc_simulate").argtypes == argtypes
    assert F.TIMER_NMPC_SIM == 21
