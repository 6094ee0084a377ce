"""kp_validate / Ksysid.val_candidates, valNplot_model, select_model on the device against the oracle with the SAME model
matrices: ko.val_model / ko.val_model_loaded followed by ko.get_error(..., scale).

Tolerances: trajectories 1e-9 absolute (the standing rollout tolerance for stable models, test_gpu_models.py); mean, rmse,
euclid_mean and unscaled_euclid_mean 1e-9 absolute; nrmse 1e-9 relative.  Every oracle rollout compared is asserted finite
and bounded first.

Dispatch regimes of kp_validate_kernel (test_every_dispatch_regime_and_chunk_boundary): one wave (N <= 64, and nfull <= 64
for a nonlinear dictionary) or four waves; the model staged in LDS or read from memory; each with trials of T_q = 1, 2,
chunk - 1, chunk, chunk + 1 rows, chunk = KP_VALIDATE_CHUNK = 128.

The divergence case of the issue (spectral radius 1.5 over 400 steps) does not leave the finite range - 1.5^400 is 1e70 and
the oracle stays finite too - so the test keeps that trial, where the status must stay 0 as the oracle says, and adds a
trial of 2000 steps (1.5^1751 overflows a double), where status and non-finite metrics are asserted."""
import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from test_gpu_fit import make_basis
from tests._loaded_system import make_trials

TC = F.VALIDATE_CHUNK
TOL = 1e-9


def _cut(v, a, b):
    return {k: np.asarray(x)[a:b] for k, x in v.items()}


def _toy(ctx, mt, nd=0, nw=0, deg=2):
    """Ksysid of the toy pendulum, candidates = least-squares fits on 700, 1000 and all snapshot pairs, and its oracle
    dictionary."""
    trials = make_trials(10, 150, nw=max(nw, 1), seed=21)
    if nw == 0:
        trials = [{k: x for k, x in t.items() if k != "w"} for t in trials]
    ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[deg],
                    delays=nd, loaded=nw > 0)
    extract = {"nonlinear": ks.get_NLmodel, "bilinear": ks.get_BLmodel, "linear": ks.get_model}[mt]
    cands = []
    for cnt in (700, 1000, None):
        sub = {k: F.fcol(np.asarray(x)[:cnt]) for k, x in ks.snapshotPairs.items()}
        kd = ks.get_Koopman(sub)
        kd["beta"] = sub["beta"]
        cands.append(extract(kd))
    dic = ko.build_dictionary(mt, ks.params["nzeta"], 1, ["poly"], [deg])
    assert dic.N == ks.params["N"]
    return ks, cands, dic


@pytest.fixture(scope="module")
def toys(ctx):
    cache = {}

    def get(mt, nd=0, nw=0):
        if (mt, nd, nw) not in cache:
            cache[(mt, nd, nw)] = _toy(ctx, mt, nd, nw)
        return cache[(mt, nd, nw)]
    return get


def _oracle_pair(ks, dic, model, v):
    nd, mt = ks.params["nd"], ks.model_type
    r = (ko.val_model_loaded if ks.loaded else ko.val_model)(dic, model, v, nd, mt)
    assert np.isfinite(r["sim_y"]).all() and np.abs(r["sim_y"]).max() < 10.0          # a stable model: the oracle itself is sound
    return r["sim_y"], ko.get_error(r["sim_y"], r["real_y"], ks.params["scale"])


def _check_pair(tab, i, q, ysim, e, sim=True):
    for k in ("mean", "rmse"):
        assert np.abs(tab[k][i, q] - e[k]).max() < TOL, (k, i, q)
    assert abs(tab["euclid_mean"][i, q] - e["euclid_mean"]) < TOL, (i, q)
    assert abs(tab["unscaled_euclid_mean"][i, q] - e["unscaled_euclid_mean"]) < TOL, (i, q)
    assert np.all(np.abs(tab["nrmse"][i, q] - e["nrmse"]) <= TOL * np.abs(e["nrmse"])), (i, q)
    assert not tab["diverged"][i, q]
    if sim:
        assert tab["sim"][i][q].shape == ysim.shape and np.abs(tab["sim"][i][q] - ysim).max() < TOL, (i, q)


def _same_table(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("mean", "rmse", "nrmse", "euclid_mean", "unscaled_euclid_mean", "diverged"))


def _four_trials(ks):
    v0, v1 = ks.valdata
    return [v0, _cut(v1, 0, 97), _cut(v0, 20, 61), _cut(v1, 10, 140)]


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [0, 1])
@pytest.mark.parametrize("mt", ["linear", "bilinear", "nonlinear"])
def test_table_matches_the_oracle_for_every_candidate_and_trial(toys, mt, nd):
    """3 distinct candidates x 4 distinct trials of unequal lengths: a swapped model or trial index shows."""
    ks, cands, dic = toys(mt, nd)
    trials = _four_trials(ks)
    tab = ks.val_candidates(cands, trials, want_sim=True)
    assert tab["mean"].shape == (3, 4, 2) and tab["euclid_mean"].shape == (3, 4) and "lasso" not in tab
    ref = [[_oracle_pair(ks, dic, mo, v) for v in trials] for mo in cands]
    for i in range(3):
        for q in range(4):
            _check_pair(tab, i, q, *ref[i][q])
    # the candidates and the trials do differ by far more than the tolerance
    em = np.array([[ref[i][q][1]["euclid_mean"] for q in range(4)] for i in range(3)])
    assert np.abs(em[0] - em[2]).min() > 1e-6 and np.abs(em[:, 0] - em[:, 1]).min() > 1e-6
    quiet = ks.val_candidates(cands, trials)
    assert "sim" not in quiet and _same_table(quiet, tab)


def _random_case(ctx, mt, nzeta, m, seed):
    """A random stable model on a poly-2 dictionary of nzeta states, with n = nzeta outputs (nd = 0)."""
    rng = np.random.default_rng(seed)
    dic = ko.build_dictionary(mt, nzeta, m, ["poly"], [2])
    basis = make_basis(ctx, dic)
    N = dic.N
    models = []
    for s in (0.8, 0.6):
        if mt == "nonlinear":
            models.append({"Kf": s * rng.standard_normal((nzeta, N)) / (2.0 * np.sqrt(N))})
        else:
            A = s * np.linalg.qr(rng.standard_normal((N, N)))[0]
            B = 0.1 * rng.standard_normal((N, m)) if mt == "linear" else 0.001 * rng.standard_normal((N, N * m))
            models.append({"A": A, "B": B, "C": np.hstack([np.eye(nzeta), np.zeros((nzeta, N - nzeta))])})
    return dic, basis, models, rng


@pytest.mark.gpu
@pytest.mark.parametrize("mt,nzeta,m,waves,staged", [
    ("linear", 3, 2, 1, True), ("bilinear", 3, 2, 1, True), ("nonlinear", 2, 1, 1, True),     # N = 10, 10, 10 (nfull 10)
    ("linear", 10, 2, 4, True),                                                                 # N = 66
    ("nonlinear", 8, 3, 4, True),                                                               # N = nfull = 78
    ("bilinear", 10, 4, 4, False),                                                              # N = 66: 5 x 66 x 66 doubles > 160 KB
    ("bilinear", 8, 10, 1, False)])                                                             # N = 45: 11 x 45 x 45 doubles > 160 KB
def test_every_dispatch_regime_and_chunk_boundary(ctx, mt, nzeta, m, waves, staged):
    dic, basis, models, rng = _random_case(ctx, mt, nzeta, m, 5)
    N, n = dic.N, nzeta
    assert (1 if N <= 64 else 4) == waves
    model_doubles = nzeta * N if mt == "nonlinear" else N * N + (N * N * m if mt == "bilinear" else N * m)
    assert (model_doubles * 8 < 140 * 1024) == staged and (staged or model_doubles * 8 > 160 * 1024)
    lens = [1, 2, TC - 1, TC, TC + 1]
    trials = [{"t": np.arange(T) * 0.1, "y": rng.uniform(-1, 1, (T, n)), "u": rng.uniform(-1, 1, (T, m))} for T in lens]
    fac = rng.uniform(0.5, 2.0, n)
    sc = {"y_factor": fac, "y_offset": rng.uniform(-1, 1, n)}
    mods = [mo["Kf"] for mo in models] if mt == "nonlinear" else [(mo["A"], mo["B"]) for mo in models]
    packed = [(v["y"][0], v["u"], v["y"], None) for v in trials]
    err, st, sim = ctx.validate(basis, mt, mods, packed, n, 0, fac, want_sim=True)
    assert err.shape == (2, 5, 3 * n + 2) and not st.any()
    for i, mo in enumerate(models):
        for q, v in enumerate(trials):
            r = ko.val_model(dic, mo, v, 0, mt)
            assert np.isfinite(r["sim_y"]).all() and np.abs(r["sim_y"]).max() < 10.0
            with np.errstate(invalid="ignore"):
                e = ko.get_error(r["sim_y"], r["real_y"], sc)
            assert np.abs(sim[i][q] - r["sim_y"]).max() < TOL, (i, q)
            got = err[i, q]
            assert np.abs(got[:n] - e["mean"]).max() < TOL and np.abs(got[n:2 * n] - e["rmse"]).max() < TOL, (i, q)
            assert abs(got[3 * n] - e["euclid_mean"]) < TOL and abs(got[3 * n + 1] - e["unscaled_euclid_mean"]) < TOL, (i, q)
            if lens[q] == 1:                                   # one row: no error, and 0 / 0 for nrmse
                assert not got[:2 * n].any() and got[3 * n] == 0.0 and got[3 * n + 1] == 0.0 and np.isnan(got[2 * n:3 * n]).all()
                assert np.array_equal(sim[i][q], v["y"])
            else:
                assert np.all(np.abs(got[2 * n:3 * n] - e["nrmse"]) <= TOL * np.abs(e["nrmse"])), (i, q)
    err2, _, _ = ctx.validate(basis, mt, mods, packed, n, 0, fac)
    assert np.array_equal(err2, err, equal_nan=True)
    basis.close()


def _random_walk_load(v, seed):
    rng = np.random.default_rng(seed)
    w = np.asarray(v["w"], dtype=np.float64)
    out = dict(v)
    out["w"] = np.clip(w[0] + np.cumsum(rng.uniform(-0.1, 0.1, w.shape), axis=0), -1.0, 1.0)
    assert np.all(np.any(out["w"][1:] != out["w"][:-1], axis=1))          # the load changes at every step
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("mt", ["linear", "bilinear", "nonlinear"])
def test_loaded_models_with_constant_and_per_step_loads(toys, mt, nw):
    ks, cands, dic = toys(mt, 0, nw)
    assert ks.params["nw"] == nw and cands[0]["Kf" if mt == "nonlinear" else "A"].shape[1] == dic.N * (nw + 1)
    v0, v1 = ks.valdata
    const = [v0, _cut(v1, 5, 102)]
    walk = [_random_walk_load(v0, 3), _random_walk_load(_cut(v1, 5, 102), 4)]
    trials = const + walk
    tab = ks.val_candidates(cands, trials, want_sim=True)
    for i, mo in enumerate(cands):
        for q, v in enumerate(trials):
            _check_pair(tab, i, q, *_oracle_pair(ks, dic, mo, v))
    # a constant load: the existing per-trial path (A_eff on the host, one launch per trial)
    val = {"linear": ks.val_model, "bilinear": ks.val_BLmodel, "nonlinear": ks.val_NLmodel}[mt]
    for i, mo in enumerate(cands):
        for q, v in enumerate(const):
            res = val(mo, v)
            assert np.abs(tab["sim"][i][q] - res["sim"]["y"]).max() < TOL
            assert abs(tab["euclid_mean"][i, q] - res["error"]["euclid_mean"]) < TOL
            assert np.abs(tab["rmse"][i, q] - res["error"]["rmse"]).max() < TOL
    assert _same_table(ks.val_candidates(cands, trials), tab)


@pytest.mark.gpu
@pytest.mark.parametrize("mt,nw", [("linear", 0), ("nonlinear", 0), ("bilinear", 2)])
def test_a_pair_has_the_same_bits_alone_first_and_last_in_a_batch(toys, mt, nw):
    ks, cands, _ = toys(mt, 0, nw)
    trials = _four_trials(ks) if nw == 0 else [ks.valdata[0], _cut(ks.valdata[1], 0, 97), _random_walk_load(ks.valdata[1], 9)]
    mo, v = cands[1], trials[1]
    alone = ks.val_candidates(mo, v, want_sim=True)
    first = ks.val_candidates([mo, cands[0], cands[2]], [v] + trials[2:] + trials[:1], want_sim=True)
    last = ks.val_candidates([cands[2], cands[0], mo], trials[2:] + trials[:1] + [v], want_sim=True)
    again = ks.val_candidates([cands[2], cands[0], mo], trials[2:] + trials[:1] + [v], want_sim=True)
    for k in ("mean", "rmse", "nrmse", "euclid_mean", "unscaled_euclid_mean"):
        assert np.array_equal(alone[k][0, 0], first[k][0, 0]) and np.array_equal(alone[k][0, 0], last[k][-1, -1]), k
    assert np.array_equal(alone["sim"][0][0], first["sim"][0][0]) and np.array_equal(alone["sim"][0][0], last["sim"][-1][-1])
    assert _same_table(again, last)
    assert all(np.array_equal(a, b) for ra, rb in zip(again["sim"], last["sim"]) for a, b in zip(ra, rb))


@pytest.mark.gpu
def test_a_diverged_candidate_is_flagged_and_leaves_its_neighbour_alone(toys):
    ks, cands, dic = toys("linear", 0, 0)
    stable = cands[2]
    rho = np.abs(np.linalg.eigvals(stable["A"])).max()
    wild = dict(stable, A=np.asfortranarray(stable["A"] * (1.5 / rho)))
    v = ks.valdata[0]
    reps = -(-2001 // len(v["t"]))
    long = {"t": 0.1 * np.arange(2001), "y": np.tile(v["y"], (reps, 1))[:2001], "u": np.tile(v["u"], (reps, 1))[:2001]}
    trials = [_cut(long, 0, 401), long]                             # 400 steps: 1.5^400 ~ 1e70, finite; 2000 steps: overflow
    with np.errstate(all="ignore"):
        r400 = ko.val_model(dic, wild, trials[0], 0, "linear")["sim_y"]
        r2000 = ko.val_model(dic, wild, trials[1], 0, "linear")["sim_y"]
    assert np.isfinite(r400).all() and np.abs(r400).max() > 1e60 and not np.isfinite(r2000).all()
    tab = ks.val_candidates([wild, stable], trials, want_sim=True)
    assert tab["diverged"].tolist() == [[False, True], [False, False]]
    assert np.isfinite(tab["euclid_mean"][0, 0]) and tab["euclid_mean"][0, 0] > 1e50
    for k in ("mean", "rmse", "euclid_mean", "unscaled_euclid_mean"):
        assert not np.isfinite(tab[k][0, 1]).any(), k
    assert not np.isfinite(tab["sim"][0][1]).all()
    ref = ks.val_candidates(stable, trials, want_sim=True)
    for k in ("mean", "rmse", "nrmse", "euclid_mean", "unscaled_euclid_mean"):
        assert np.array_equal(tab[k][1], ref[k][0]), k
    for q in range(2):
        _check_pair(tab, 1, q, *_oracle_pair(ks, dic, stable, trials[q]))
    keep = ks.candidates, ks.model
    try:
        ks.candidates = [wild, stable]
        best, _ = ks.select_model(table=tab)
        assert best == 1 and ks.model is stable
        with pytest.raises(ValueError):
            ks.select_model(table=ks.val_candidates([wild, wild], trials[1:]))
    finally:
        ks.candidates, ks.model = keep


def _refused(ctx, call):
    with pytest.raises(F.KoopmanHipError) as ei:
        call()
    assert ei.value.code == F.KP_ERR_ARG and "kp_validate" in str(ei.value)
    return str(ei.value)


@pytest.mark.gpu
def test_refusals_are_argument_errors_and_leave_the_context_usable(ctx, toys):
    ks, cands, dic = toys("linear", 0, 0)
    v = ks.valdata[0]
    fac = ks.params["scale"]["y_factor"]
    mods = [(cands[0]["A"], cands[0]["B"])]
    good = [(v["y"][0], v["u"], v["y"], None)]
    want = ctx.validate(ks.basis_dev, "linear", mods, good, 2, 0, fac)[0]

    def usable():
        assert np.array_equal(ctx.validate(ks.basis_dev, "linear", mods, good, 2, 0, fac)[0], want)

    bil = make_basis(ctx, ko.build_dictionary("bilinear", 2, 1, ["poly"], [2]))
    assert "model type" in _refused(ctx, lambda: ctx.validate(bil, "linear", mods, good, 2, 0, fac))
    bil.close()
    usable()
    N = dic.N
    wide = [(v["y"][0], v["u"], np.zeros((len(v["t"]), N + 1)), None)]
    assert "outputs" in _refused(ctx, lambda: ctx.validate(ks.basis_dev, "linear", mods, wide, N + 1, 0, np.ones(N + 1)))
    usable()
    empty = good + [(v["y"][0], np.zeros((0, 1)), np.zeros((0, 2)), None)]
    assert "empty" in _refused(ctx, lambda: ctx.validate(ks.basis_dev, "linear", mods, empty, 2, 0, fac))
    usable()


@pytest.mark.gpu
def test_a_model_beyond_the_lds_limit_is_refused_and_val_candidates_falls_back(ctx):
    """120 inputs and 20 outputs: one chunk of 128 steps - 120 x 128 inputs, 2 x 20 x 129 outputs - with the state vectors and
    the error sums is 20 922 doubles, more than 160 KB.  The per-trial rollout kernel, with its shorter chunks, takes it."""
    rng = np.random.default_rng(2)
    n, m = 20, 120
    trials = [{"t": 0.1 * np.arange(T), "y": rng.uniform(-1, 1, (T, n)), "u": rng.uniform(-1, 1, (T, m))} for T in (60, 60, 33, 47)]
    ks = kra.Ksysid({"train": trials[:2], "val": trials[2:]}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[1])
    N = ks.params["N"]
    assert N == n + 1
    mo = {"A": np.asfortranarray(0.9 * np.linalg.qr(rng.standard_normal((N, N)))[0]), "B": np.asfortranarray(0.05 * rng.standard_normal((N, m))),
          "C": np.hstack([np.eye(n), np.zeros((n, 1))]), "lasso": 7.0}
    packed = [(v["y"][0], v["u"], v["y"], None) for v in ks.valdata]
    msg = _refused(ctx, lambda: ctx.validate(ks.basis_dev, "linear", [(mo["A"], mo["B"])], packed, n, 0, ks.params["scale"]["y_factor"]))
    assert "LDS" in msg
    tab = ks.val_candidates(mo, want_sim=True)
    assert tab["mean"].shape == (1, 2, n)
    for q, v in enumerate(ks.valdata):
        res = ks.val_model(mo, v)
        assert np.isfinite(res["sim"]["y"]).all() and np.abs(res["sim"]["y"][1:]).max() > 1e-3
        assert np.array_equal(tab["sim"][0][q], res["sim"]["y"]) and not tab["diverged"][0, q]
        for k in ("mean", "rmse", "nrmse", "euclid_mean"):
            assert np.array_equal(tab[k][0, q], res["error"][k]), k
        assert tab["unscaled_euclid_mean"][0, q] == res["error"]["unscaled"]["euclid_mean"]
    assert np.array_equal(tab["lasso"], [7.0])


def _same_results(res, e, ref):
    assert set(res) == set(ref) and set(e) == set(ref["error"])
    assert np.array_equal(res["t"], ref["t"])
    for side in ("sim", "real"):
        assert set(res[side]) == set(ref[side])
        for k in res[side]:
            if (side, k) == ("sim", "y"):
                assert np.abs(res[side][k] - ref[side][k]).max() < TOL
            else:
                assert np.array_equal(res[side][k], ref[side][k]), (side, k)
    re = ref["error"]
    for k in ("abs", "mean", "rmse", "euclid"):
        assert np.abs(e[k] - re[k]).max() < TOL, k
    assert abs(e["euclid_mean"] - re["euclid_mean"]) < TOL
    assert np.all(np.abs(e["nrmse"] - re["nrmse"]) <= TOL * np.abs(re["nrmse"]))
    assert set(e["unscaled"]) == set(re["unscaled"])
    assert np.abs(e["unscaled"]["euclid"] - re["unscaled"]["euclid"]).max() < TOL
    assert abs(e["unscaled"]["euclid_mean"] - re["unscaled"]["euclid_mean"]) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("mt,nw", [("linear", 0), ("bilinear", 0), ("nonlinear", 0), ("linear", 1)])
def test_valnplot_model_equals_the_loop_of_val_calls(toys, mt, nw):
    ks, cands, _ = toys(mt, 0, nw)
    val = {"linear": ks.val_model, "bilinear": ks.val_BLmodel, "nonlinear": ks.val_NLmodel}[mt]
    keep = ks.candidates, ks.model
    try:
        ks.candidates = cands
        for mid, mo in ((None, cands[0]), (2, cands[2])):
            results, err = ks.valNplot_model(mid)
            refs = [val(mo, v) for v in ks.valdata]
            assert len(results) == len(err) == len(refs) == 2
            for res, e, ref in zip(results, err, refs):
                assert res["error"] is e
                _same_results(res, e, ref)
    finally:
        ks.candidates, ks.model = keep


@pytest.mark.gpu
def test_train_models_then_select_model_keeps_the_best_candidate(ctx):
    trials = [{k: x for k, x in t.items() if k != "w"} for t in make_trials(10, 150, nw=1, seed=21)]
    ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[2],
                    lasso=[0.3, 1.0, 10.0])
    ks.train_models()
    assert len(ks.candidates) == 3 and ks.model is ks.candidates[0]
    best, tab = ks.select_model()
    assert np.array_equal(tab["lasso"], [0.3, 1.0, 10.0]) and tab["euclid_mean"].shape == (3, 2) and not tab["diverged"].any()
    score = tab["euclid_mean"].mean(axis=1)
    assert len(set(score)) == 3 and best == int(np.argmin(score)) and ks.model is ks.candidates[best]
    for metric in ("rmse", "nrmse", "mean", "unscaled_euclid_mean"):
        b2, t2 = ks.select_model(metric, tab)
        assert t2 is tab and b2 == int(np.argmin(tab[metric].reshape(3, -1).mean(axis=1))) and ks.model is ks.candidates[b2]
