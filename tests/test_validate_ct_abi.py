"""CPU test: kp_validate_ct is declared in include/koopman_hip_validate.h (not in koopman_hip.h, which the MATLAB gateway
covers one for one), bound in _ffi.VALIDATE_SIGNATURES with the argument count of its declaration, and exported by the
built library; the constants of the header are those of _ffi."""
import os
import re

import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    ge.build()
    from koopman_realizations_amd import _ffi
    return _ffi


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_kp_validate_ct_is_declared_bound_and_exported(built):
    hdr = _header("koopman_hip_validate.h")
    declared = set(re.findall(r"^int\s+(kp_[a-z_A-Z0-9]+)\s*\(", hdr, re.M))
    assert declared == {"kp_validate", "kp_validate_ct"} == set(built.VALIDATE_SIGNATURES)
    assert "kp_validate_ct" not in _header("koopman_hip.h") and "kp_validate_ct" not in built.SIGNATURES
    lib = built.lib()
    assert lib.kp_validate_ct is not None
    # one ctypes argument per declared parameter: kp_validate's, then Ts, rtol, atol, and the two step counts at the end
    decl = re.search(r"^int\s+kp_validate_ct\s*\(([^;]*)\)\s*;", hdr, re.M).group(1)
    nargs = len(decl.split(","))
    res, args = built.VALIDATE_SIGNATURES["kp_validate_ct"]
    assert len(args) == nargs == len(built.VALIDATE_SIGNATURES["kp_validate"][1]) + 5
    assert lib.kp_validate_ct.argtypes == args and lib.kp_validate_ct.restype is res


def test_the_constants_of_the_header_are_those_of_the_python_mirror(built):
    hdr = _header("koopman_hip_validate.h")
    for name, val in (("KP_VALIDATE_CHUNK", built.VALIDATE_CHUNK), ("KP_VALIDATE_CT_CHUNK", built.VALIDATE_CT_CHUNK),
                      ("KP_VALIDATE_CT_STAGE", built.VALIDATE_CT_STAGE)):
        assert int(re.search(name + r"\s*=\s*(\d+)", hdr).group(1)) == val, name
