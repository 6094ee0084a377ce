"""CPU tests of the closed-loop layer: Kmpc.resample_ref (Kmpc.m:390-399) and the C ABI of include/koopman_hip_sim.h."""
import os
import re
import types

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    ge.build()
    from koopman_realizations_amd import _ffi
    return _ffi


def test_resample_ref_is_interp1_at_the_sampling_time(built):
    from koopman_realizations_amd.kmpc import Kmpc
    Ts = 0.05
    me = types.SimpleNamespace(params={"Ts": Ts})                 # resample_ref reads nothing else
    rng = np.random.default_rng(2)
    t = np.concatenate([[0.0], np.sort(rng.uniform(0.01, 0.97, 17)), [0.98]])    # non-uniform; 0.98 is no multiple of Ts
    y = rng.standard_normal((t.size, 3))
    out = Kmpc.resample_ref(me, {"t": t, "y": y})
    tr = np.arange(20) * Ts                                        # 0 : Ts : 0.98 ends at 0.95
    assert out.shape == (20, 3)
    for j in range(3):
        assert np.array_equal(out[:, j], np.interp(tr, t, y[:, j]))
    assert np.array_equal(out[0], y[0])
    # an end time that IS a multiple of Ts keeps its last sample; a single column may come as a vector
    t2 = np.array([0.0, 0.13, 0.5, 1.0])
    out2 = Kmpc.resample_ref(me, {"t": t2, "y": np.array([0.0, 1.0, -1.0, 2.0])})
    assert out2.shape == (21, 1) and out2[-1, 0] == 2.0
    assert np.array_equal(out2[:, 0], np.interp(np.arange(21) * Ts, t2, [0.0, 1.0, -1.0, 2.0]))
    # samples already at Ts come back as they are
    t3 = np.arange(7) * Ts
    y3 = rng.standard_normal((7, 2))
    assert np.abs(Kmpc.resample_ref(me, {"t": t3, "y": y3}) - y3).max() < 1e-15


def test_every_symbol_of_the_sim_header_is_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "koopman_hip_sim.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)               # declarations only: the comments name other entry points
    declared = set(re.findall(r"\b(kp_[a-z_A-Z0-9]+)\s*\(", hdr))
    assert declared == {"kp_mpc_simulate"}, declared
    assert declared == set(built.SIM_SIGNATURES), declared ^ set(built.SIM_SIGNATURES)
    lib = built.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn is not None and fn.argtypes == built.SIM_SIGNATURES[name][1]
    assert not set(built.SIM_SIGNATURES) & set(built.SIGNATURES)
