"""kp_validate_ct / Context.validate_ct and the continuous-time route of Ksysid.val_candidates, valNplot_model and
select_model, against the host restatement with the SAME model matrices: tests/_ct_reference.rollout_host (arm.dopri45 over
every sample interval, the input held) followed by the oracle's get_error.

Tolerances, the project's standing ones: trajectories 1e-10 relative to the host dopri45 with equal accepted / rejected step
counts (test_gpu_continuous.py); mean, rmse, euclid_mean and unscaled_euclid_mean 1e-9 absolute, nrmse 1e-9 relative
(test_gpu_validate.py).  Every host rollout compared is asserted finite and bounded (< 10) first.

Models: stable random continuous models as test_gpu_continuous.py builds them - A = -2 I + randn / sqrt(N), B = 0.1 randn,
bilinear B = 1e-3 randn, nonlinear Kf = randn / (2 sqrt(N)) with -I on the state columns - with Ts = 0.1.

Dispatch regimes of kp_validate_ct_kernel (test_every_dispatch_regime_and_chunk_boundary): 64 threads (N <= 64, and
nfull <= 64 for a nonlinear dictionary) or 256; the matrix - A, Kf, or the bilinear A + sum_i u_i B_i of a sample - in LDS
(at most KP_VALIDATE_CT_STAGE doubles) or in memory (a bilinear one in the pair's slice of device scratch); each with trials
of 1, 2, chunk - 1, chunk and chunk + 1 rows, chunk = KP_VALIDATE_CT_CHUNK = 32.  A matrix beyond the staging limit is wider
than 64, so the 64-thread kernel always has it staged."""
import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from _ct_reference import arm_trials, bilinear_rhs, linear_rhs, nonlinear_rhs, rollout_host
from test_gpu_fit import make_basis

pytestmark = pytest.mark.gpu

TC = F.VALIDATE_CT_CHUNK
TS = 0.1
TOL = 1e-9
METRICS = ("mean", "rmse", "nrmse", "euclid_mean", "unscaled_euclid_mean")


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _cut(v, a, b):
    return {k: np.asarray(x)[a:b] for k, x in v.items()}


def ct_case(mt, nzeta, m, seed, nmod=2):
    """Stable random continuous models on a poly-2 dictionary of nzeta states and m inputs, n = nzeta outputs."""
    rng = np.random.default_rng(seed)
    dic = ko.build_dictionary(mt, nzeta, m, ["poly"], [2])
    N = dic.N
    models = []
    for s in (1.0, 0.7)[:nmod]:
        if mt == "nonlinear":
            Kf = s * rng.standard_normal((nzeta, N)) / (2.0 * np.sqrt(N))
            Kf[:, :nzeta] -= np.eye(nzeta)
            models.append({"Kf": Kf})
        else:
            A = -2.0 * np.eye(N) + s * rng.standard_normal((N, N)) / np.sqrt(N)
            B = 0.1 * rng.standard_normal((N, m)) if mt == "linear" else 1e-3 * rng.standard_normal((N, N * m))
            models.append({"A": A, "B": B})
    return dic, models, rng


def random_trials(rng, lens, n, m):
    return [{"t": TS * np.arange(T), "y": rng.uniform(-1, 1, (T, n)), "u": rng.uniform(-1, 1, (T, m))} for T in lens]


def host_pair(dic, mt, mo, v, sc):
    """The host yardstick of one pair: (ysim, naccept, nreject, errors)."""
    n = v["y"].shape[1]
    T = v["y"].shape[0]
    if mt == "nonlinear":
        Z, na, nr = rollout_host(nonlinear_rhs(dic, mo["Kf"]), v["y"][0], v["u"], TS)
    else:
        z0 = ko.econ_full(dic, v["y"][0][None, :])[0]
        Z, na, nr = rollout_host((linear_rhs if mt == "linear" else bilinear_rhs)(mo["A"], mo["B"]), z0, v["u"], TS)
    assert Z.shape[0] == T and np.isfinite(Z).all() and np.abs(Z).max() < 10.0        # a stable model: the yardstick itself is sound
    ys = Z[:, :n].copy()
    ys[0] = v["y"][0]                                                                    # Ksysid.m:1654
    with np.errstate(invalid="ignore"):
        e = ko.get_error(ys, v["y"], sc)
    return ys, na, nr, e


def pack(models, trials, mt):
    mods = [mo["Kf"] for mo in models] if mt == "nonlinear" else [(mo["A"], mo["B"]) for mo in models]
    return mods, [(v["y"][0], v["u"], v["y"], None) for v in trials]


def check_pair(err, st, sim, na, nr, i, q, ref, n, one_row=False):
    ys, na_h, nr_h, e = ref
    got = err[i, q]
    assert st[i, q] == 0 and (na[i, q], nr[i, q]) == (na_h, nr_h), (i, q, na[i, q], nr[i, q], na_h, nr_h)
    if sim is not None:
        assert sim[i][q].shape == ys.shape and np.array_equal(sim[i][q][0], ys[0])
        assert _rel(sim[i][q], ys) <= 1e-10, (i, q, _rel(sim[i][q], ys))
    assert np.abs(got[:n] - e["mean"]).max() < TOL and np.abs(got[n:2 * n] - e["rmse"]).max() < TOL, (i, q)
    assert abs(got[3 * n] - e["euclid_mean"]) < TOL and abs(got[3 * n + 1] - e["unscaled_euclid_mean"]) < TOL, (i, q)
    if one_row:                                                # one row: no error, and 0 / 0 for nrmse
        assert not got[:2 * n].any() and got[3 * n] == 0.0 and got[3 * n + 1] == 0.0 and np.isnan(got[2 * n:3 * n]).all()
        assert (na[i, q], nr[i, q]) == (0, 0)
    else:
        assert np.all(np.abs(got[2 * n:3 * n] - e["nrmse"]) <= TOL * np.abs(e["nrmse"])), (i, q)


# ---- 1. the table against the host ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt,lens", [("linear", (97, 41, 70, 30)), ("bilinear", (97, 41, 70, 30)), ("nonlinear", (33, 17, 28, 22))])
def test_table_matches_the_host_for_every_candidate_and_trial(ctx, mt, lens):
    """2 distinct models x 4 distinct trials of unequal lengths, 3 states and 2 inputs (N = 10; nonlinear: 21): a swapped
    model or trial index shows."""
    dic, models, rng = ct_case(mt, 3, 2, 7)
    n, m = 3, 2
    assert dic.N == (21 if mt == "nonlinear" else 10)
    basis = make_basis(ctx, dic)
    trials = random_trials(rng, lens, n, m)
    fac = rng.uniform(0.5, 2.0, n)
    sc = {"y_factor": fac, "y_offset": rng.uniform(-1, 1, n)}
    mods, packed = pack(models, trials, mt)
    err, st, sim, na, nr = ctx.validate_ct(basis, mt, mods, packed, n, fac, TS, want_sim=True)
    assert err.shape == (2, 4, 3 * n + 2) and st.shape == na.shape == nr.shape == (2, 4) and not st.any()
    ref = [[host_pair(dic, mt, mo, v, sc) for v in trials] for mo in models]
    for i in range(2):
        for q in range(4):
            check_pair(err, st, sim, na, nr, i, q, ref[i][q], n)
    # the candidates and the trials do differ by far more than the tolerance
    em = np.array([[ref[i][q][3]["euclid_mean"] for q in range(4)] for i in range(2)])
    assert np.abs(em[0] - em[1]).min() > 1e-6 and np.abs(em[:, 0] - em[:, 1]).min() > 1e-6
    quiet = ctx.validate_ct(basis, mt, mods, packed, n, fac, TS)
    assert quiet[2] is None
    assert np.array_equal(quiet[0], err) and all(np.array_equal(a, b) for a, b in zip(quiet[1:2] + quiet[3:], (st, na, nr)))
    basis.close()


def test_a_stiff_model_rejects_steps_as_the_host_does(ctx):
    """Rates near -600 with MaxStep = Ts / 10 = 0.01: a step that grows to h = 0.01 has h |lambda| = 6, outside the stability
    region of the pair (about 3.3), so the error test fails again and again and the shrink-then-halve branch of the step
    control runs - as on the host, step for step."""
    dic, _, rng = ct_case("linear", 3, 2, 3)
    n, m, N = 3, 2, dic.N
    basis = make_basis(ctx, dic)
    mo = {"A": -600.0 * np.eye(N) + rng.standard_normal((N, N)) / np.sqrt(N), "B": 20.0 * rng.standard_normal((N, m))}
    trials = random_trials(rng, (40, 25), n, m)
    fac = rng.uniform(0.5, 2.0, n)
    sc = {"y_factor": fac, "y_offset": rng.uniform(-1, 1, n)}
    ref = [host_pair(dic, "linear", mo, v, sc) for v in trials]
    assert all(r[2] > 10 for r in ref)                         # rejected steps on the host
    err, st, sim, na, nr = ctx.validate_ct(basis, "linear", *pack([mo], trials, "linear"), n, fac, TS, want_sim=True)
    for q in range(2):
        check_pair(err, st, sim, na, nr, 0, q, ref[q], n)
    basis.close()


# ---- 2. every dispatch regime and chunk boundary ----------------------------------------------------------------------------
REGIMES = [
    ("linear", 3, 2, 1, True, 2), ("bilinear", 3, 2, 1, True, 2), ("nonlinear", 3, 2, 1, True, 2),   # N = 10, 10, 21 (nfull 21)
    ("linear", 10, 2, 4, True, 2),                                                                     # N = 66
    ("nonlinear", 8, 3, 4, True, 2),                                                                   # N = nfull = 78
    ("bilinear", 12, 2, 4, False, 2),                      # N = 91: 8 281 doubles > 8 192, A + sum u_i B_i in device scratch
    ("linear", 12, 2, 4, False, 2),                        # N = 91: A read from memory
    ("nonlinear", 28, 1, 4, False, 1)]                     # N = 465: Kf 28 x 465 = 13 020 doubles read from memory


@pytest.mark.parametrize("mt,nzeta,m,waves,staged,nmod", REGIMES)
def test_every_dispatch_regime_and_chunk_boundary(ctx, mt, nzeta, m, waves, staged, nmod):
    dic, models, rng = ct_case(mt, nzeta, m, 5, nmod)
    N, n = dic.N, nzeta
    basis = make_basis(ctx, dic)
    assert (1 if N <= 64 and (mt != "nonlinear" or basis.nfull <= 64) else 4) == waves
    assert ((nzeta * N if mt == "nonlinear" else N * N) <= F.VALIDATE_CT_STAGE) == staged
    lens = [1, 2, TC - 1, TC, TC + 1]
    trials = random_trials(rng, lens, n, m)
    fac = rng.uniform(0.5, 2.0, n)
    sc = {"y_factor": fac, "y_offset": rng.uniform(-1, 1, n)}
    mods, packed = pack(models, trials, mt)
    err, st, sim, na, nr = ctx.validate_ct(basis, mt, mods, packed, n, fac, TS, want_sim=True)
    assert err.shape == (nmod, 5, 3 * n + 2) and not st.any()
    for i, mo in enumerate(models):
        for q, v in enumerate(trials):
            check_pair(err, st, sim, na, nr, i, q, host_pair(dic, mt, mo, v, sc), n, one_row=lens[q] == 1)
            if lens[q] == 1:
                assert np.array_equal(sim[i][q], v["y"])
    err2, st2, _, na2, nr2 = ctx.validate_ct(basis, mt, mods, packed, n, fac, TS)
    assert np.array_equal(err2, err, equal_nan=True) and np.array_equal(na2, na) and np.array_equal(nr2, nr) and not st2.any()
    basis.close()


@pytest.mark.parametrize("mt,nzeta,m", [r[:3] for r in REGIMES])
def test_the_table_and_the_rollout_are_one_integrator(ctx, mt, nzeta, m):
    """kp_validate_ct_kernel and kp_ct_rollout_kernel run the same code (kp_ct_step.h) on the same start bits - the matrix
    models' z_0 is the device lift the per-trial val_model route takes - so the samples behind row 0 and the step counts of a
    pair are those of one kp_rollout_ct / kp_rollout_nl_ct call, bit for bit.  One model, trials of 2 and chunk + 1 rows (a
    chunk boundary inside the second) in every regime of the dispatch test."""
    dic, models, rng = ct_case(mt, nzeta, m, 5, 1)
    n, mo = nzeta, models[0]
    basis = make_basis(ctx, dic)
    trials = random_trials(rng, (2, TC + 1), n, m)
    _, st, sim, na, nr = ctx.validate_ct(basis, mt, *pack([mo], trials, mt), n, np.ones(n), TS, want_sim=True)
    assert not st.any()
    for q, v in enumerate(trials):
        if mt == "nonlinear":
            Z, a, r, s = ctx.rollout_nl_ct(basis, mo["Kf"], v["y"][0], v["u"], TS)
        else:
            z0 = basis.lift(F.LIFT_ECON, v["y"][0])[0]
            Z, a, r, s = ctx.rollout_ct(mt, mo["A"], mo["B"], z0, v["u"], n, TS)
        assert s == 0 and a > 0 and Z.shape == sim[0][q].shape
        assert np.array_equal(sim[0][q][1:], Z[1:]) and (na[0, q], nr[0, q]) == (a, r), (q, na[0, q], nr[0, q], a, r)
    basis.close()


# ---- 3. independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt,nzeta,m", [("linear", 3, 2), ("nonlinear", 3, 2), ("bilinear", 12, 2)])
def test_a_pair_has_the_same_bits_alone_first_and_last_in_a_batch(ctx, mt, nzeta, m):
    """The bilinear case is beyond the LDS staging: every pair has its own slice of the scratch buffer."""
    dic, models, rng = ct_case(mt, nzeta, m, 11)
    n = nzeta
    basis = make_basis(ctx, dic)
    trials = random_trials(rng, (TC + 9, 12, 40), n, m)
    fac = rng.uniform(0.5, 2.0, n)
    third = {k: 0.9 * x for k, x in models[0].items()}
    mo, v = models[1], trials[1]

    def run(ms, vs):
        return ctx.validate_ct(basis, mt, *pack(ms, vs, mt), n, fac, TS, want_sim=True)

    alone = run([mo], [v])
    first = run([mo, models[0], third], [v, trials[2], trials[0]])
    last = run([third, models[0], mo], [trials[2], trials[0], v])
    again = run([third, models[0], mo], [trials[2], trials[0], v])
    assert alone[3][0, 0] > 0 and not alone[1].any()
    for k in (0, 1, 3, 4):                                      # err, status, naccept, nreject
        assert np.array_equal(alone[k][0, 0], first[k][0, 0]) and np.array_equal(alone[k][0, 0], last[k][-1, -1]), k
        assert np.array_equal(again[k], last[k]), k
    assert np.array_equal(alone[2][0][0], first[2][0][0]) and np.array_equal(alone[2][0][0], last[2][-1][-1])
    assert all(np.array_equal(a, b) for ra, rb in zip(again[2], last[2]) for a, b in zip(ra, rb))
    # the other pairs of the batch are other numbers
    assert not np.array_equal(first[0][0, 0], first[0][1, 0]) and not np.array_equal(first[0][0, 0], first[0][0, 1])
    basis.close()


# ---- Ksysid objects on small random data ---------------------------------------------------------------------------------
def _small_ksysid(ctx, n, m, lens, seed, deg=2):
    rng = np.random.default_rng(seed)
    trials = random_trials(rng, lens, n, m)
    ks = kra.Ksysid({"train": trials[:2], "val": trials[2:]}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[deg],
                    time_type="continuous")
    assert abs(ks.params["Ts"] - TS) < 1e-12
    return ks, rng


# ---- 4. divergence is data, not an error -----------------------------------------------------------------------------------
def test_a_diverged_candidate_is_flagged_and_leaves_its_neighbour_alone(ctx):
    """A = 30 I with Ts = 0.1 over 400 rows: e^(3 j) leaves the doubles near row 237.  z_0 holds the constant observable 1, so
    the state itself overflows at j >= 236.6, and the stage sums before it: their largest term, |a_52 k_2| = 11.6 x 30 |z|,
    from e^(3 j) > 5.2e305, j >= 234.4.  The first failing row is therefore one of 235 .. 237."""
    ks, rng = _small_ksysid(ctx, 3, 2, (60, 60, 400, 150), 4)
    N, m, n = ks.params["N"], 2, 3
    assert N == 10
    stable = {"A": -2.0 * np.eye(N) + rng.standard_normal((N, N)) / np.sqrt(N), "B": 0.1 * rng.standard_normal((N, m)), "lasso": 1.0}
    wild = {"A": 30.0 * np.eye(N), "B": stable["B"], "lasso": 2.0}
    trials = ks.valdata
    # the host integrator on the wild model ends outside the finite range too
    _, yreal, ureal, zetareal = ks._val_common(trials[0])
    with np.errstate(all="ignore"):
        Zh, _, _ = rollout_host(linear_rhs(wild["A"], wild["B"]), ks.lift.econ_full(zetareal[0]), ureal, TS)
    assert np.isfinite(Zh[:230]).all() and not np.isfinite(Zh[-1]).any()
    tab = ks.val_candidates([wild, stable], trials, want_sim=True)              # KP_OK: no exception
    assert tab["diverged"].tolist() == [[True, False], [False, False]]
    y = tab["sim"][0][0]
    bad = np.flatnonzero(~np.isfinite(y).all(axis=1))
    assert 235 <= bad[0] <= 237 and np.isfinite(y[:bad[0]]).all() and np.isnan(y[bad[0]:]).all()
    for k in ("mean", "rmse", "euclid_mean", "unscaled_euclid_mean"):
        assert not np.isfinite(tab[k][0, 0]).any(), k
    # 150 rows: e^(3 x 149) ~ 1e194 is finite, so that pair did not diverge (its squared errors do overflow: rmse is Inf)
    assert np.isfinite(tab["sim"][0][1]).all() and np.isfinite(tab["mean"][0, 1]).all() and tab["mean"][0, 1].max() > 1e100
    ref = ks.val_candidates(stable, trials, want_sim=True)
    for k in METRICS:
        assert np.array_equal(tab[k][1], ref[k][0]), k
    assert all(np.array_equal(a, b) for a, b in zip(tab["sim"][1], ref["sim"][0]))
    assert np.isfinite(ref["euclid_mean"]).all() and not ref["diverged"].any()
    # the per-trial loop reports the same rollout as diverged
    loop = ks._val_table_loop([wild], trials[:1], True)
    assert loop["diverged"].tolist() == [[True]]
    ks.candidates = [wild, stable]
    best, _ = ks.select_model(table=tab)
    assert best == 1 and ks.model is stable
    best, t2 = ks.select_model("rmse")
    assert best == 1 and t2["diverged"].tolist() == [[True, False], [False, False]]


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(F.KoopmanHipError) as ei:
        call()
    assert ei.value.code == F.KP_ERR_ARG and "kp_validate_ct" in str(ei.value)
    return str(ei.value)


def test_refusals_are_argument_errors_and_leave_the_context_usable(ctx):
    dic, models, rng = ct_case("linear", 3, 2, 13)
    n, m, N = 3, 2, dic.N
    basis = make_basis(ctx, dic)
    trials = random_trials(rng, (30, 9), n, m)
    fac = np.ones(n)
    mods, good = pack(models, trials, "linear")
    want = ctx.validate_ct(basis, "linear", mods, good, n, fac, TS)

    def usable():
        got = ctx.validate_ct(basis, "linear", mods, good, n, fac, TS)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3]) and not got[1].any()

    assert "loaded" in _refused(lambda: ctx.validate_ct(basis, "linear", mods, good, n, fac, TS, nw=1))
    usable()
    assert "positive" in _refused(lambda: ctx.validate_ct(basis, "linear", mods, good, n, fac, 0.0))
    usable()
    assert "positive" in _refused(lambda: ctx.validate_ct(basis, "linear", mods, good, n, fac, TS, rtol=0.0))
    usable()
    assert "positive" in _refused(lambda: ctx.validate_ct(basis, "linear", mods, good, n, fac, TS, atol=float("nan")))
    usable()
    wide = [(v["y"][0], v["u"], np.zeros((len(v["t"]), N + 1)), None) for v in trials]
    assert "outputs" in _refused(lambda: ctx.validate_ct(basis, "linear", mods, wide, N + 1, np.ones(N + 1), TS))
    usable()
    basis.close()


def test_a_shape_beyond_the_lds_limit_is_refused_and_val_candidates_falls_back(ctx):
    """650 inputs: one chunk of 32 samples holds 650 x 32 inputs = 20 800 doubles, more than the 160 KB of LDS by itself.
    kp_rollout_ct, which shortens its chunks to what fits, takes it: val_candidates falls back to the per-trial loop."""
    n, m = 2, 650
    ks, rng = _small_ksysid(ctx, n, m, (40, 40, 33, 21), 2, deg=1)
    N = ks.params["N"]
    assert N == n + 1
    mo = {"A": -2.0 * np.eye(N) + rng.standard_normal((N, N)) / np.sqrt(N), "B": 0.02 * rng.standard_normal((N, m)), "lasso": 7.0}
    packed = [(v["y"][0], v["u"], v["y"], None) for v in ks.valdata]
    msg = _refused(lambda: ctx.validate_ct(ks.basis_dev, "linear", [(mo["A"], mo["B"])], packed, n, ks.params["scale"]["y_factor"], TS))
    assert "LDS" in msg
    tab = ks.val_candidates(mo, want_sim=True)
    assert set(tab) == {"mean", "rmse", "nrmse", "euclid_mean", "unscaled_euclid_mean", "diverged", "sim", "lasso"}
    assert tab["mean"].shape == (1, 2, n)
    for q, v in enumerate(ks.valdata):
        res = ks.val_model(mo, v)
        assert np.isfinite(res["sim"]["y"]).all() and np.abs(res["sim"]["y"][1:]).max() > 1e-3
        assert np.array_equal(tab["sim"][0][q], res["sim"]["y"]) and not tab["diverged"][0, q]
        for k in ("mean", "rmse", "nrmse", "euclid_mean"):
            assert np.array_equal(tab[k][0, q], res["error"][k]), k
        assert tab["unscaled_euclid_mean"][0, q] == res["error"]["unscaled"]["euclid_mean"]
    assert np.array_equal(tab["lasso"], [7.0])


# ---- 6. end to end, and the route ------------------------------------------------------------------------------------------
def _same_as_loop(tab, loop, nmod, ntr):
    for i in range(nmod):
        for q in range(ntr):
            assert np.isfinite(loop["sim"][i][q]).all() and np.abs(loop["sim"][i][q]).max() < 10.0
            assert _rel(tab["sim"][i][q], loop["sim"][i][q]) <= 1e-10, (i, q)
            for k in ("mean", "rmse"):
                assert np.abs(tab[k][i, q] - loop[k][i, q]).max() < TOL, (k, i, q)
            for k in ("euclid_mean", "unscaled_euclid_mean"):
                assert abs(tab[k][i, q] - loop[k][i, q]) < TOL, (k, i, q)
            assert np.all(np.abs(tab["nrmse"][i, q] - loop["nrmse"][i, q]) <= TOL * np.abs(loop["nrmse"][i, q])), (i, q)
    assert not tab["diverged"].any() and not loop["diverged"].any()


def _no_rollout(*a, **k):
    raise AssertionError("the per-trial continuous rollout was called")


def test_val_candidates_of_a_continuous_lasso_grid_is_one_call_and_equals_the_loop(ctx, golden, monkeypatch):
    train, val = arm_trials(golden)
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[2], dim_red=True,
                    time_type="continuous", lasso=[1e4, 2e4]).train_models()
    assert len(ks.candidates) == 2
    v = ks.valdata[0]
    trials = [v, _cut(v, 0, 97), _cut(v, 40, 40 + TC), _cut(v, 150, 333)]
    tab = ks.val_candidates(ks.candidates, trials, want_sim=True)
    loop = ks._val_table_loop(ks.candidates, trials, True)
    assert tab["mean"].shape == (2, 4, 6) and np.array_equal(tab["lasso"], [1e4, 2e4])
    _same_as_loop(tab, loop, 2, 4)
    assert np.abs(tab["euclid_mean"][:, 0] - tab["euclid_mean"][:, 1]).min() > 1e-6    # the trials do differ (the two lasso values
    #                                                                                    of this configuration give the same model)
    # the route: no per-trial rollout is left in val_candidates, valNplot_model and select_model
    monkeypatch.setattr(ks.ctx, "rollout_ct", _no_rollout)
    monkeypatch.setattr(ks.ctx, "rollout_nl_ct", _no_rollout)
    with pytest.raises(AssertionError):
        ks.val_model(ks.candidates[0], v)
    again = ks.val_candidates(ks.candidates, trials, want_sim=True)
    assert all(np.array_equal(again[k], tab[k]) for k in METRICS)
    results, errs = ks.valNplot_model(0)
    assert len(results) == 1 and np.array_equal(results[0]["sim"]["y"], tab["sim"][0][0])
    assert errs[0]["euclid_mean"] == tab["euclid_mean"][0, 0]
    best, t2 = ks.select_model("rmse")
    assert best == int(np.argmin(t2["rmse"].reshape(2, -1).mean(axis=1))) and ks.model is ks.candidates[best]


@pytest.mark.parametrize("mt,rows", [("bilinear", 200), ("nonlinear", 100)])
def test_bilinear_and_nonlinear_arm_models_equal_the_loop(ctx, golden, monkeypatch, mt, rows):
    """The poly-3 dim_red arm models of test_gpu_continuous.py's ct_models."""
    train, val = arm_trials(golden)
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[3], dim_red=True,
                    time_type="continuous")
    ks.train_models()
    v = _cut(ks.valdata[0], 0, rows)
    trials = [v, _cut(v, 10, 10 + TC + 1)]
    tab = ks.val_candidates(ks.model, trials, want_sim=True)
    loop = ks._val_table_loop([ks.model], trials, True)
    _same_as_loop(tab, loop, 1, 2)
    monkeypatch.setattr(ks.ctx, "rollout_ct", _no_rollout)
    monkeypatch.setattr(ks.ctx, "rollout_nl_ct", _no_rollout)
    again = ks.val_candidates(ks.model, trials)
    assert all(np.array_equal(again[k], tab[k]) for k in METRICS)
