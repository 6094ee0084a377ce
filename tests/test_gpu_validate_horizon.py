"""kp_validate_horizon / Context.validate_horizon / Ksysid.val_horizon, horizon_slice and select_model(horizon=...) on the
device against tests/_horizon_reference.py, the numpy restatement of the definition (checked against the oracle's one-step
maps in tests/test_horizon_host.py), with the SAME model matrices.

Tolerance: 1e-9 absolute on every metric, the project's standing rollout tolerance (tests/test_gpu_validate.py), for H <= 20;
every comparison first asserts, on the restatement, that the predictions are finite and |yhat| <= 10, so that an absolute
bound means something.

The tile width S_T (64, 32 or 16) and whether the model rows were staged in LDS are read back from
kp_timer_get(F.TIMER_HORIZON_TILE) = 1000 x staged + S_T; _lds_rule restates the rule of include/koopman_hip_horizon.h."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from test_gpu_fit import make_basis
from tests import _horizon_reference as hr
from tests._loaded_system import make_trials
from tests.test_matio import write_mat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
METRICS = ("mean", "rmse", "euclid_mean", "unscaled_euclid_mean")


def _pad4(x):
    return (x + 3) // 4 * 4


def _lds_rule(mt, N, m, n, nz, nfull, k_pcs):
    """(S_T, staged) by the header's rule: the widest tile whose columns fit 160 KB, the model staged when it fits beside."""
    nvars = nz + (m if mt == "nonlinear" else 0)
    K = {"linear": N + m, "bilinear": N * (1 + m), "nonlinear": N}[mt]
    R = nz if mt == "nonlinear" else N
    col = _pad4(nvars) + 2 + (_pad4(nfull) + 2 if k_pcs else 0) + _pad4(K) + 2 + _pad4(R) + 2 + F.HORIZON_CHUNK * (m + n + 2)
    for S in (64, 32, 16):
        fixed = (n + 1) // 2 * 2 + S * col + F.HORIZON_CHUNK
        if fixed * 8 <= 160 * 1024:
            return S, (fixed + _pad4(R) * _pad4(K)) * 8 <= 160 * 1024
    return 0, False


def _mods(mt, models):
    return [mo["Kf"] for mo in models] if mt == "nonlinear" else [(mo["A"], mo["B"]) for mo in models]


def _reference(dic, models, trials, n, fac, H, stride):
    """The restatement's table; its predictions asserted finite and bounded."""
    tab, res = hr.horizon_table(dic, models, trials, n, fac, H, stride)
    for row in res:
        for r in row:
            assert np.isfinite(r["yhat"]).all() and (r["yhat"].size == 0 or np.abs(r["yhat"]).max() <= 10.0)
    return tab


def _close(err, st, ns, ref, n):
    assert np.array_equal(ns, ref["starts"]) and not st.any()
    got = {"mean": err[..., :n], "rmse": err[..., n:2 * n], "euclid_mean": err[..., 2 * n], "unscaled_euclid_mean": err[..., 2 * n + 1]}
    for k in METRICS:
        assert got[k].shape == ref[k].shape, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        print(k, "max |device - restatement| =", np.nanmax(np.abs(got[k] - ref[k]), initial=0.0))
        assert np.nanmax(np.abs(got[k] - ref[k]), initial=0.0) < TOL, k


def _cut(v, a, b):
    return {k: np.asarray(x)[a:b] for k, x in v.items()}


# ---- 1. parity with the restatement on fitted toy models -----------------------------------------------------------------
def _toy(ctx, mt, nd):
    """Ksysid of the toy pendulum; three candidates: the least-squares model with A (or Kf) scaled by 1, 1.001 and 0.98."""
    trials = [{k: x for k, x in t.items() if k != "w"} for t in make_trials(10, 150, nw=1, seed=21)]
    ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[2], delays=nd)
    ks.train_models()
    base = ks.model
    key = "Kf" if mt == "nonlinear" else "A"
    cands = [dict(base, **{key: np.asfortranarray(np.asarray(base[key]) * s)}) for s in (1.0, 1.001, 0.98)]
    dic = ko.build_dictionary(mt, ks.params["nzeta"], 1, ["poly"], [2])
    assert dic.N == ks.params["N"]
    return ks, cands, dic


@pytest.fixture(scope="module")
def toys(ctx):
    cache = {}

    def get(mt, nd=0):
        if (mt, nd) not in cache:
            cache[(mt, nd)] = _toy(ctx, mt, nd)
        return cache[(mt, nd)]
    return get


def _zu(ks, v):
    _, _, u, zeta = ks._val_common(v)
    return zeta, u


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [0, 1])
@pytest.mark.parametrize("mt", ["linear", "bilinear", "nonlinear"])
def test_table_matches_the_restatement(toys, mt, nd):
    ks, cands, dic = toys(mt, nd)
    n, fac = ks.params["n"], ks.params["scale"]["y_factor"]
    vals = [ks.valdata[0], _cut(ks.valdata[1], 0, 97)]                       # two trials of different length
    for stride in (1, 3):
        tab = ks.val_horizon(8, cands, vals, stride=stride)
        ref = _reference(dic, cands, [_zu(ks, v) for v in vals], n, fac, 8, stride)
        assert tab["mean"].shape == (3, 2, 8, n) and tab["euclid_mean"].shape == (3, 2, 8) and tab["horizon"] == 8 and tab["stride"] == stride
        assert np.array_equal(tab["starts"], ref["starts"]) and not tab["diverged"].any() and "lasso" in tab
        assert np.array_equal(tab["starts"], [(len(z) - 1 - 8) // stride + 1 for z, _ in (_zu(ks, v) for v in vals)])
        for k in METRICS:
            print(mt, nd, stride, k, np.abs(tab[k] - ref[k]).max())
            assert np.abs(tab[k] - ref[k]).max() < TOL, k
        # the comparison tells the candidates apart
        e8 = ref["euclid_mean"][:, :, 7]
        assert min(np.abs(e8[0] - e8[1]).min(), np.abs(e8[0] - e8[2]).min(), np.abs(e8[1] - e8[2]).min()) > 1e-6
        # pooled: all starts of all trials together
        w = ref["starts"] / ref["starts"].sum()
        assert np.abs(tab["pooled"]["euclid_mean"] - np.einsum("q,iqh->ih", w, ref["euclid_mean"])).max() < TOL
        assert np.abs(tab["pooled"]["rmse"] - np.sqrt(np.einsum("q,iqhc->ihc", w, ref["rmse"] ** 2))).max() < TOL
        assert tab["pooled"]["mean"].shape == (3, 8, n)


# ---- 2. shapes where the kernel can go wrong ----------------------------------------------------------------------------------
def _synthetic(ctx, mt, N, m, seed):
    """A model that is stable by construction on the dictionary [x, x^2 .. x^(N-1), 1] of one state: 0.9 x orthogonal A, small B."""
    rng = np.random.default_rng(seed)
    dic = ko.build_dictionary(mt, 1, m, ["poly"], [N - 1])
    assert dic.N == N
    basis = make_basis(ctx, dic)
    models = []
    for s in (0.9, 0.7):
        A = s * np.linalg.qr(rng.standard_normal((N, N)))[0]
        B = 0.1 * rng.standard_normal((N, m)) if mt == "linear" else 0.001 * rng.standard_normal((N, N * m))
        models.append({"A": A, "B": B})
    return dic, basis, models, rng


def _trial(rng, T, nz, m):
    return rng.uniform(-1, 1, (T, nz)), rng.uniform(-1, 1, (T, m))


def _tile(ctx):
    code = int(ctx.timer(F.TIMER_HORIZON_TILE))
    return code % 1000, code // 1000 == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mt,N,m", [("linear", 3, 1), ("linear", 5, 3), ("bilinear", 5, 1), ("linear", 17, 3), ("bilinear", 17, 3),
                                    ("linear", 34, 1), ("bilinear", 34, 3)])
def test_odd_sizes_and_every_tile_boundary(ctx, mt, N, m):
    dic, basis, models, rng = _synthetic(ctx, mt, N, m, 7 * N + m)
    n, fac, H = 1, np.array([1.7]), 6
    ST, staged = _lds_rule(mt, N, m, n, 1, N, 0)
    assert staged
    lens = [S + H for S in (1, ST - 1, ST, ST + 1, 2 * ST + 3)]
    trials = [_trial(rng, T, 1, m) for T in lens]
    err, ns, st = ctx.validate_horizon(basis, mt, _mods(mt, models), trials, n, fac, H)
    assert _tile(ctx) == (ST, True)
    assert ns.tolist() == [1, ST - 1, ST, ST + 1, 2 * ST + 3]
    _close(err, st, ns, _reference(dic, models, trials, n, fac, H, 1), n)
    # a stride that is no divisor of anything, on the same trials
    err3, ns3, st3 = ctx.validate_horizon(basis, mt, _mods(mt, models), trials, n, fac, H, stride=5)
    _close(err3, st3, ns3, _reference(dic, models, trials, n, fac, H, 5), n)
    basis.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mt", ["linear", "bilinear"])
def test_horizon_one_the_whole_trial_and_a_trial_without_a_start(ctx, mt):
    dic, basis, models, rng = _synthetic(ctx, mt, 5, 3, 11)
    n, fac = 1, np.array([0.6])
    trials = [_trial(rng, T, 1, 3) for T in (21, 9, 30)]
    mods = _mods(mt, models)
    # H = 1: every row but the last starts a prediction
    err, ns, st = ctx.validate_horizon(basis, mt, mods, trials, n, fac, 1)
    assert ns.tolist() == [20, 8, 29] and err.shape == (2, 3, 1, 4)
    _close(err, st, ns, _reference(dic, models, trials, n, fac, 1, 1), n)
    # H = T - 1 of the first trial: exactly one start there; the second trial is too short, the third has 10 starts
    err, ns, st = ctx.validate_horizon(basis, mt, mods, trials, n, fac, 20)
    assert ns.tolist() == [1, 0, 10] and np.isnan(err[:, 1]).all() and not st.any()
    _close(err, st, ns, _reference(dic, models, trials, n, fac, 20, 1), n)
    # ... and the others are what they are without it, bit for bit
    err2, ns2, _ = ctx.validate_horizon(basis, mt, mods, [trials[0], trials[2]], n, fac, 20)
    assert ns2.tolist() == [1, 10] and np.array_equal(err2, err[:, [0, 2]])
    basis.close()


@pytest.mark.gpu
def test_a_model_staged_in_lds_and_one_too_large_to_stage(ctx):
    n, fac, H = 1, np.array([1.0]), 5
    for m, want in ((3, (64, True)), (12, (32, False))):
        assert _lds_rule("bilinear", 34, m, n, 1, 34, 0) == want
        dic, basis, models, rng = _synthetic(ctx, "bilinear", 34, m, 3 + m)
        ST = want[0]
        trials = [_trial(rng, T, 1, m) for T in (ST + 2 + H, 7 + H)]        # short trials: two tiles and one
        err, ns, st = ctx.validate_horizon(basis, "bilinear", _mods("bilinear", models), trials, n, fac, H)
        assert _tile(ctx) == want
        _close(err, st, ns, _reference(dic, models, trials, n, fac, H, 1), n)
        basis.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim_red", [False, True])
@pytest.mark.parametrize("mt", ["nonlinear", "linear"])
def test_a_dictionary_with_and_without_pcs(ctx, mt, dim_red):
    rng = np.random.default_rng(5)
    nz, m, n = 3, 2, 2
    pairs = {"alpha": rng.uniform(-1, 1, (400, nz)), "u": rng.uniform(-1, 1, (400, m))}
    dic = ko.build_dictionary(mt, nz, m, ["poly"], [3], pairs=pairs, dim_red=dim_red)
    basis = make_basis(ctx, dic)
    N = dic.N
    assert (dic.pcs is not None) == dim_red
    models = []
    for s in (0.8, 0.6):
        if mt == "nonlinear":
            models.append({"Kf": s * rng.standard_normal((nz, N)) / (2.0 * np.sqrt(N))})
        else:
            models.append({"A": s * np.linalg.qr(rng.standard_normal((N, N)))[0], "B": 0.1 * rng.standard_normal((N, m))})
    fac, H = np.array([2.0, 0.5]), 7
    ST, _ = _lds_rule(mt, N, m, n, nz, dic.basis.nfull, 0 if dic.pcs is None else dic.pcs.shape[1])
    trials = [_trial(rng, T, nz, m) for T in (ST + 1 + H, 5 + H, H)]
    err, ns, st = ctx.validate_horizon(basis, mt, _mods(mt, models), trials, n, fac, H)
    assert _tile(ctx)[0] == ST and ns.tolist() == [ST + 1, 5, 0]
    _close(err, st, ns, _reference(dic, models, trials, n, fac, H, 1), n)
    basis.close()


# ---- 3. consistency with kp_validate --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mt", ["linear", "bilinear", "nonlinear"])
def test_one_start_over_the_whole_trial_sums_to_the_table_of_val_candidates(toys, mt):
    """One start (s = 0, H = T - 1): sum_h euclid_mean[h] = T x val_candidates' euclid_mean of the pair - row 0 of val_* is
    exact, and val_* divides by T - to 1e-9 T; the same for mean |d|."""
    ks, cands, _ = toys(mt, 0)
    T = 21
    v = _cut(ks.valdata[0], 10, 10 + T)
    hz = ks.val_horizon(T - 1, cands, v)
    full = ks.val_candidates(cands, v)
    assert hz["starts"].tolist() == [1] and not hz["diverged"].any() and not full["diverged"].any()
    assert np.abs(hz["euclid_mean"][:, 0].sum(axis=1) - T * full["euclid_mean"][:, 0]).max() < TOL * T
    assert np.abs(hz["unscaled_euclid_mean"][:, 0].sum(axis=1) - T * full["unscaled_euclid_mean"][:, 0]).max() < TOL * T
    assert np.abs(hz["mean"][:, 0].sum(axis=1) - T * full["mean"][:, 0]).max() < TOL * T
    assert full["euclid_mean"].min() > 1e-6                                    # the sums are of something


# ---- 4. batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mt", ["linear", "bilinear", "nonlinear"])
def test_a_pair_has_the_same_bits_alone_first_and_last_in_a_batch(toys, mt):
    ks, cands, _ = toys(mt, 0)
    v0, v1 = ks.valdata
    trials = [v0, _cut(v1, 0, 97), _cut(v0, 20, 61), _cut(v1, 10, 140)]
    mo, v = cands[1], trials[1]
    alone = ks.val_horizon(8, mo, v)
    first = ks.val_horizon(8, [mo, cands[0], cands[2]], [v] + trials[2:] + trials[:1])
    last = ks.val_horizon(8, [cands[2], cands[0], mo], trials[2:] + trials[:1] + [v])
    other = ks.val_horizon(8, [cands[0], mo], [trials[3], v, trials[0], trials[2], trials[0]])        # another nmod and ntr
    again = ks.val_horizon(8, [cands[2], cands[0], mo], trials[2:] + trials[:1] + [v])
    for k in METRICS:
        assert np.array_equal(alone[k][0, 0], first[k][0, 0]) and np.array_equal(alone[k][0, 0], last[k][-1, -1]), k
        assert np.array_equal(alone[k][0, 0], other[k][1, 1]) and np.array_equal(again[k], last[k]), k
        assert np.isfinite(alone[k]).all() and alone[k].any()
    assert alone["starts"].tolist() == [89] and last["starts"].tolist() == [33, 122, 142, 89]        # one tile and several


# ---- 5. divergence -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_diverged_candidate_is_flagged_and_its_neighbours_keep_their_bits(toys):
    """A scaled by 50: the prediction leaves the finite range after some 180 steps (50^181 > 1.8e308), so the horizon is 200."""
    ks, cands, dic = toys("linear", 0)
    stable = cands[0]
    wild = dict(stable, A=np.asfortranarray(np.asarray(stable["A"]) * 50.0))
    v = ks.valdata[0]
    reps = -(-231 // len(v["t"]))
    long = {"t": 0.1 * np.arange(231), "y": np.tile(v["y"], (reps, 1))[:231], "u": np.tile(v["u"], (reps, 1))[:231]}
    H = 200
    with np.errstate(all="ignore"):
        yw = hr.predictions(dic, wild, *_zu(ks, long), 2, H)[0]
    assert not np.isfinite(yw[:, -1]).all() and np.isfinite(yw[:, 0]).all()
    tab = ks.val_horizon(H, [stable, wild, cands[2]], [long, ks.valdata[1]])
    assert tab["starts"].tolist() == [31, 0]
    assert tab["diverged"].tolist() == [[False, False], [True, False], [False, False]]
    assert np.isfinite(tab["euclid_mean"][1, 0, 0]) and not np.isfinite(tab["euclid_mean"][1, 0, -1])
    assert not np.isfinite(tab["rmse"][1, 0, -1]).any()
    ref = ks.val_horizon(H, [stable, cands[2]], [long, ks.valdata[1]])
    for k in METRICS:
        assert np.array_equal(tab[k][[0, 2]], ref[k], equal_nan=True) and np.isfinite(ref[k][:, 0]).all(), k
    keep = ks.candidates, ks.model
    try:
        ks.candidates = [stable, wild, cands[2]]
        best, _ = ks.select_model("rmse", table=ks.horizon_slice(tab, H))
        assert best != 1
    finally:
        ks.candidates, ks.model = keep


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def _refused(call, word=None):
    with pytest.raises(F.KoopmanHipError) as ei:
        call()
    assert ei.value.code == F.KP_ERR_ARG and (word is None or word in str(ei.value)), str(ei.value)
    return str(ei.value)


@pytest.mark.gpu
def test_refusals_are_argument_errors_and_leave_the_context_usable(ctx, toys):
    ks, cands, dic = toys("linear", 0)
    N, n, nz, m = dic.N, 2, 2, 1
    fac = np.ascontiguousarray(ks.params["scale"]["y_factor"], dtype=np.float64)
    mods = [(cands[0]["A"], cands[0]["B"])]
    good = [_zu(ks, ks.valdata[0])]
    want = ctx.validate_horizon(ks.basis_dev, "linear", mods, good, n, fac, 5)[0]
    assert np.isfinite(want).all()

    def usable():
        assert np.array_equal(ctx.validate_horizon(ks.basis_dev, "linear", mods, good, n, fac, 5)[0], want)

    for H, stride in ((0, 1), (-3, 1), (5, 0), (5, -1)):
        _refused(lambda: ctx.validate_horizon(ks.basis_dev, "linear", mods, good, n, fac, H, stride), "at least 1")
        usable()
    bil = make_basis(ctx, ko.build_dictionary("bilinear", 2, 1, ["poly"], [2]))
    _refused(lambda: ctx.validate_horizon(bil, "linear", mods, good, n, fac, 5), "model type")
    bil.close()
    usable()
    wide = [(np.zeros((30, nz)), np.zeros((30, m)))]
    _refused(lambda: ctx.validate_horizon(ks.basis_dev, "linear", mods, wide, N + 1, np.ones(N + 1), 5), "outputs")
    usable()
    _refused(lambda: ctx.validate_horizon(ks.basis_dev, "linear", mods, wide, nz + 1, np.ones(nz + 1), 5), "outputs")
    usable()
    empty = good + [(np.zeros((0, nz)), np.zeros((0, m)))]
    _refused(lambda: ctx.validate_horizon(ks.basis_dev, "linear", mods, empty, n, fac, 5), "empty")
    usable()

    # the raw entry point: counts, a dictionary of other dimensions, NULL pointers
    A = np.ascontiguousarray(np.asarray(cands[0]["A"]).T); B = np.ascontiguousarray(np.asarray(cands[0]["B"]).T)
    Z, U = F.fcol(good[0][0]), F.fcol(good[0][1])
    off = np.array([0, Z.shape[0]], dtype=np.int64)
    err = np.zeros((1, 1, 5, 2 * n + 2)); ns = np.zeros(1, dtype=np.int64); st = np.zeros(1, dtype=np.int32)
    i64 = C.POINTER(C.c_int64)

    def raw(**kw):
        a = dict(basis=ks.basis_dev.handle, N=N, m=m, n=n, nz=nz, nmod=1, A=F.dptr(A), B=F.dptr(B), ntr=1, off=off.ctypes.data_as(i64),
                 Z=F.dptr(Z), U=F.dptr(U), fac=F.dptr(fac), H=5, stride=1, err=F.dptr(err), ns=ns.ctypes.data_as(i64),
                 st=st.ctypes.data_as(F.c_ip))
        a.update(kw)
        F.check(F.lib().kp_validate_horizon(ctx._h, a["basis"], F.MODEL["linear"], a["N"], a["m"], a["n"], a["nz"], a["nmod"], a["A"], a["B"],
                                            a["ntr"], a["off"], a["Z"], a["U"], a["fac"], a["H"], a["stride"], a["err"], a["ns"], a["st"]),
                ctx._h)

    raw()
    assert np.array_equal(err, want)
    for kw in (dict(nmod=0), dict(ntr=0), dict(N=N + 1), dict(m=m + 1), dict(nz=nz + 1), dict(basis=None), dict(A=None), dict(B=None),
               dict(off=None), dict(Z=None), dict(U=None), dict(fac=None), dict(err=None), dict(ns=None), dict(st=None)):
        _refused(lambda: raw(**kw), "kp_validate_horizon")
        usable()


@pytest.mark.gpu
def test_a_shape_beyond_the_lds_limit_is_refused_with_a_message(ctx):
    """150 inputs: a column of the tile is 6 + 158 + 6 doubles and 8 x 153 staged ones; 16 columns are more than 160 KB."""
    m, n = 150, 1
    assert _lds_rule("linear", 3, m, n, 1, 3, 0) == (0, False)
    dic, basis, models, rng = _synthetic(ctx, "linear", 3, m, 1)
    msg = _refused(lambda: ctx.validate_horizon(basis, "linear", _mods("linear", models), [_trial(rng, 12, 1, m)], n, np.ones(1), 4), "LDS")
    assert "kp_validate_horizon" in msg
    basis.close()


@pytest.mark.gpu
def test_continuous_and_loaded_objects_are_declined(ctx):
    trials = make_trials(6, 60, nw=1, seed=3)
    plain = [{k: x for k, x in t.items() if k != "w"} for t in trials]
    ct = kra.Ksysid({"train": plain[:4], "val": plain[4:]}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[2],
                    time_type="continuous")
    with pytest.raises(NotImplementedError, match="continuous"):
        ct.val_horizon(5, {"A": np.eye(6), "B": np.zeros((6, 1))})
    ld = kra.Ksysid({"train": trials[:4], "val": trials[4:]}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[2], loaded=True)
    with pytest.raises(NotImplementedError, match="loaded"):
        ld.val_horizon(5, {"A": np.eye(12), "B": np.zeros((12, 1))})
    with pytest.raises(NotImplementedError, match="loaded"):
        ld.select_model("rmse", horizon=5)
    # the library itself: the dictionary of a loaded object's fit is not the models' dictionary
    if ld.basis_loaded_dev is None:
        ld.train_models()
    lb = ld.basis_loaded_dev                                       # 'bilinear' over zeta with the pseudo-input [w; u]
    N = lb.N
    zu = [(ld._val_common(v)[3], np.zeros((len(ld._val_common(v)[2]), lb.m))) for v in ld.valdata]
    _refused(lambda: ctx.validate_horizon(lb, "linear", [(np.eye(N), np.zeros((N, lb.m)))], zu, 2, np.ones(2), 5), "model type")


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(ctx):
    """train_models on a three-value lasso grid, and the restatement's rmse at step 5 of every candidate."""
    raw = make_trials(10, 150, nw=1, seed=21)
    trials = [{k: x for k, x in t.items() if k != "w"} for t in raw]
    ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[2],
                    lasso=[0.3, 1.0, 10.0])
    ks.train_models()
    dic = ko.build_dictionary("linear", 2, 1, ["poly"], [2])
    ref = _reference(dic, ks.candidates, [_zu(ks, v) for v in ks.valdata], 2, ks.params["scale"]["y_factor"], 5, 1)
    score = ref["rmse"][:, :, 4].reshape(3, -1).mean(axis=1)
    order = np.argsort(score)
    assert score[order[1]] - score[order[0]] > 1e-6                       # first and second are apart
    return raw, ks, ref, score, order


@pytest.mark.gpu
def test_train_models_then_select_model_at_the_horizon(trained):
    _, ks, ref, score, order = trained
    best, tab = ks.select_model("rmse", horizon=5)
    assert best == order[0] and ks.model is ks.candidates[best] and tab["rmse"].shape == (3, 2, 2)
    assert np.abs(tab["rmse"] - ref["rmse"][:, :, 4]).max() < TOL and np.array_equal(tab["lasso"], [0.3, 1.0, 10.0])
    with pytest.raises(ValueError, match="nrmse"):
        ks.select_model("nrmse", horizon=5)
    # without a horizon: the choice of before, by the whole-trial table
    whole = ks.val_candidates()
    b0, t0 = ks.select_model("rmse")
    assert b0 == int(np.argmin(whole["rmse"].reshape(3, -1).mean(axis=1))) and np.array_equal(t0["rmse"], whole["rmse"]) and "nrmse" in t0
    assert ks.model is ks.candidates[b0]


@pytest.mark.gpu
def test_the_cli_prints_every_candidate_at_the_horizon_and_stores_the_chosen_model(trained, tmp_path):
    raw, ks, _, score, order = trained
    f = str(tmp_path / "d.mat"); out = str(tmp_path / "model.npz")
    write_mat(f, raw)
    base = [sys.executable, "-m", "koopman_realizations_amd", "sysid", f, "--model_type", "linear", "--obs_degree", "2", "--lasso", "0.3", "1", "10",
            "--metric", "rmse", "--out", out]
    r = subprocess.run(base + ["--horizon", "5"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("horizon 5: candidate ")]
    assert len(rows) == 3 and all(" rmse " in ln for ln in rows)
    got = [float(ln.split(" rmse ")[1].split()[0]) for ln in rows]
    assert np.allclose(got, score, rtol=1e-4, atol=0.0)                   # printed with six digits
    assert f"chosen by rmse at step 5: candidate {order[0]} " in r.stdout
    assert np.abs(np.load(out)["A"] - ks.candidates[order[0]]["A"]).max() < TOL
    plain = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and "horizon" not in plain.stdout and "chosen by rmse: candidate " in plain.stdout
    assert plain.stdout.splitlines()[:-2] == [ln for ln in r.stdout.splitlines() if "horizon 5" not in ln and "at step 5" not in ln][:-1]
