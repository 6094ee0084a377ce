"""CPU tests of the batched load observer: its C ABI is exported and bound, and the window planning of
Ksysid.val_observer_load / val_observer_load_sparse (koopman-realizations_amd/observer.py), with a host solve per
window, reproduces a literal transcription of the reference's loops (Ksysid.m:2046-2069, :2096-2134)."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from koopman_realizations_amd.observer import assemble_val_observer, plan_val_observer
from oracle import koopman_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    ge.build()
    from koopman_realizations_amd import _ffi
    return _ffi


def test_every_observer_header_symbol_is_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "koopman_hip_observer.h")).read()
    declared = set(re.findall(r"\b(kp_[a-z_A-Z0-9]+)\s*\(", hdr))
    assert declared == {"kp_load_observe"}
    assert declared == set(built.OBSERVER_SIGNATURES)
    lib = built.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == built.OBSERVER_SIGNATURES[name][1]
    assert not declared & set(built.SIGNATURES)          # koopman_hip.h (the gateway's set) is unchanged


def _model(mt, nzeta, m, nw, seed):
    dic = ko.build_dictionary(mt, nzeta, m, ["poly"], [2])
    NL = dic.N * (nw + 1)
    rng = np.random.default_rng(seed)
    A = 0.3 * rng.standard_normal((NL, NL))
    B = 0.3 * rng.standard_normal((NL, m if mt == "linear" else m * NL))
    return dic, {"A": A, "B": B}


def _host_observer(dic, model, mt, nw, zwin, uwin):
    """observer_load of the window (hor rows of zeta and u; pair k uses u_k), rows of the oracle, lsqlin without a pin."""
    nz, m, NL = dic.nzeta, dic.m, dic.N * (nw + 1)
    A, B = model["A"], model["B"]
    rows, rhs = [], []
    for k in range(zwin.shape[0] - 1):
        Om = np.kron(np.eye(nw + 1), ko.econ_full(dic, zwin[k][None, :])[0][:, None])
        if mt == "linear":
            rows.append(A[:nz] @ Om)
            rhs.append(zwin[k + 1, :nz] - B[:nz] @ uwin[k])
        else:
            R = A[:nz] @ Om
            for j in range(m):
                R = R + B[:nz, j * NL:(j + 1) * NL] @ Om * uwin[k, j]
            rows.append(R)
            rhs.append(zwin[k + 1, :nz])
    return ko._lsqlin_load(np.vstack(rows), np.concatenate(rhs), nw, None, pin_last_zero=False)


def _literal(dic, model, mt, nw, zeta, u, hor, update_hor=None):
    """Ksysid.m:2040-2069 (update_hor None) or :2092-2134, line by line (0-based rows)."""
    T = zeta.shape[0]
    what = np.zeros((T, nw))
    res = np.zeros(T) + 1e-6
    what_all = []
    yhor = np.zeros((hor, zeta.shape[1]))
    uhor = np.zeros((hor, u.shape[1]))
    for i in range(1, T):                                   # for i = 1 : length(valdata.t) - 1
        y_i = zeta[i - 1]
        u_i = u[i - 1] if update_hor is None else u[i]      # valdata.u(i,:) / valdata.u(i+1,:)
        yhor = np.vstack([yhor[1:], y_i])
        uhor = np.vstack([uhor[1:], u_i])
        if update_hor is None:
            what[i] = _host_observer(dic, model, mt, nw, yhor, uhor)[0]
        elif i % update_hor == 0:
            wn, rn = _host_observer(dic, model, mt, nw, yhor, uhor)
            what_all.append(wn)
            what[i] = np.mean(np.array(what_all), axis=0)
            res[i] = rn + 1e-6
        else:
            what[i] = what[i - 1]
            res[i] = res[i - 1]
    return what, res


def _planned(dic, model, mt, nw, zeta, u, hor, update_hor=None):
    zpad, upad, steps = plan_val_observer(zeta, u, hor, update_hor)
    est, rn = [], []
    for i in steps:
        s = i - 1
        e, r = _host_observer(dic, model, mt, nw, zpad[s:s + hor], upad[s:s + hor])
        est.append(e); rn.append(r)
    est = np.array(est).reshape(len(steps), nw)
    if update_hor is None:
        return assemble_val_observer(zeta.shape[0], nw, steps, est), steps
    return assemble_val_observer(zeta.shape[0], nw, steps, est, np.array(rn), sparse=True), steps


@pytest.mark.parametrize("mt,nw", [("linear", 1), ("linear", 2), ("bilinear", 1), ("bilinear", 2)])
@pytest.mark.parametrize("T,hor,update_hor", [(1, 2, 1), (2, 2, 1), (3, 12, 2), (7, 3, 5), (17, 4, 3), (25, 12, 4),
                                              (40, 2, 1), (40, 11, 5)])
def test_planning_reproduces_the_reference_loops(mt, nw, T, hor, update_hor):
    nzeta, m = 3, 2
    dic, model = _model(mt, nzeta, m, nw, seed=T * 31 + hor)
    rng = np.random.default_rng(T + 100 * hor)
    zeta = rng.uniform(-1, 1, (T, nzeta)); u = rng.uniform(-1, 1, (T, m))
    # val_observer_load
    lw, _ = _literal(dic, model, mt, nw, zeta, u, hor)
    pw, steps = _planned(dic, model, mt, nw, zeta, u, hor)
    assert np.array_equal(steps, np.arange(1, T))
    assert np.all(pw[0] == 0.0) and np.array_equal(pw, lw)
    # val_observer_load_sparse
    lw, lr = _literal(dic, model, mt, nw, zeta, u, hor, update_hor)
    (pw, pr), steps = _planned(dic, model, mt, nw, zeta, u, hor, update_hor)
    assert np.array_equal(steps, [i for i in range(1, T) if i % update_hor == 0])
    assert np.all(pw[0] == 0.0) and pr[0] == 1e-6
    assert np.abs(pw - lw).max(initial=0.0) <= 1e-14 and np.array_equal(pr, lr)


def test_planning_pads_and_shifts():
    T, hor = 6, 4
    zeta = np.arange(1, T + 1, dtype=float)[:, None] * [1.0, 10.0]
    u = np.arange(1, T + 1, dtype=float)[:, None] * 100.0
    zpad, upad, steps = plan_val_observer(zeta, u, hor)
    assert zpad.shape == (hor - 1 + T, 2) and np.all(zpad[:hor - 1] == 0) and np.array_equal(zpad[hor - 1:], zeta)
    assert np.all(upad[:hor - 1] == 0) and np.array_equal(upad[hor - 1:], u)           # u(i) beside zeta(i)
    # the window of step i = 2 holds zeta(i-hor+1 .. i) = [0, 0, zeta(1), zeta(2)]
    s = 2 - 1
    assert np.array_equal(zpad[s:s + hor, 0], [0, 0, 1, 2])
    _, ups, steps_s = plan_val_observer(zeta, u, hor, update_hor=2)
    assert np.array_equal(ups[hor - 1:hor - 1 + T - 1, 0], u[1:, 0])                  # u(i+1) beside zeta(i)
    assert np.array_equal(steps_s, [2, 4])
