"""Continuous-time models, host side (no GPU): the C ABI of include/koopman_hip_ct.h and the test-side reference the GPU tests
(test_gpu_continuous.py) compare against."""
import os
import re

import numpy as np
import pytest

from oracle import koopman_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ct_header_matches_signatures_and_exports():
    from koopman_realizations_amd import _ffi as F
    src = open(os.path.join(ROOT, "include", "koopman_hip_ct.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\bint\s+(kp_\w+)\s*\(", src))
    assert declared == set(F.CT_SIGNATURES)
    assert not declared & (set(F.SIGNATURES) | set(F.NMPC_SIGNATURES) | set(F.OBSERVER_SIGNATURES))
    lib = F.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == F.CT_SIGNATURES[name][1]


def test_dopri45_counts_its_steps():
    from koopman_realizations_amd.arm import dopri45
    st = {}
    y = dopri45(lambda t, y: -y, 0.0, 1.0, np.array([1.0]), stats=st)
    assert abs(y[0] - np.exp(-1.0)) < 1e-3
    assert st["naccept"] >= 10 and st.get("nreject", 0) >= 0     # MaxStep = span / 10
    assert np.array_equal(dopri45(lambda t, y: -y, 0.0, 1.0, np.array([1.0])), y)


@pytest.fixture(scope="module")
def linear_arm(golden, arm):
    pytest.importorskip("scipy")
    dic = ko.build_dictionary("linear", 6, 3, ["poly"], [3], arm["pairs"], dim_red=True)
    Px, Py = ko.px_py(dic, arm["pairs"])
    K = ko.koopman_ls(Px, Py)
    return dic, K


def test_host_reference_reproduces_the_discrete_recursion_for_a_linear_model(arm, linear_arm):
    """K's input rows are [0 I], so expm(Ts UT) = K' + 1e-12 I: the continuous linear model held over Ts gives back the
    discrete unprojected blocks.  Pins the host reference (scipy logm + dopri45) of the GPU tests."""
    from _ct_reference import continuous_K, discrete_recursion, linear_rhs, rollout_host
    dic, K = linear_arm
    N = K.shape[0] - 3
    Ts = float(np.mean(np.diff(np.ravel(arm["raw"]["t"]))))
    UT = continuous_K(K, Ts).T
    Ac, Bc = UT[:N, :N], UT[:N, N:]
    Ad, Bd = K.T[:N, :N], K.T[:N, N:]
    v = arm["val"]
    y = ko.scaledown(arm["scale"], "y", v["y"]); u = ko.scaledown(arm["scale"], "u", v["u"])
    z0 = ko.econ_full(dic, y[:1])[0]
    Zd = discrete_recursion(Ad, Bd, z0, u)
    Zc, nacc, nrej = rollout_host(linear_rhs(Ac, Bc), z0, u, Ts, rtol=1e-10, atol=1e-12)
    err = np.abs(Zc[:, :6] - Zd[:, :6]).max() / np.abs(Zd[:, :6]).max()
    assert err <= 1e-8, err
    assert nacc >= 10 * (len(u) - 1)
