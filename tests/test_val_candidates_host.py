"""CPU tests of the host logic around the validation table: Ksysid.select_model on hand-made tables (ranking, NaN and
diverged candidates last, nothing left) and the argument handling of Ksysid.valNplot_model (Ksysid.m:1928-1972) with
val_candidates replaced by a stub.  No device: the objects are built without the constructor."""
import numpy as np
import pytest

from koopman_realizations_amd.ksysid import Ksysid


def _bare(ncand=3, single=False):
    ks = Ksysid.__new__(Ksysid)
    ks.candidates = {"id": 0} if single else [{"id": i} for i in range(ncand)]
    ks.model = ks.candidates if single else ks.candidates[0]
    return ks


def _table(euclid, diverged=None, n=2):
    euclid = np.asarray(euclid, dtype=np.float64)
    nmod, ntr = euclid.shape
    per_out = np.repeat(euclid[:, :, None], n, axis=2)
    return {"mean": per_out.copy(), "rmse": per_out.copy(), "nrmse": per_out.copy(), "euclid_mean": euclid,
            "unscaled_euclid_mean": 3.0 * euclid,
            "diverged": np.zeros((nmod, ntr), dtype=bool) if diverged is None else np.asarray(diverged, dtype=bool)}


def test_select_model_takes_the_least_mean_over_the_trials():
    ks = _bare()
    tab = _table([[0.3, 0.5], [0.1, 0.2], [0.05, 0.6]])          # means 0.4, 0.15, 0.325: the least single entry does not win
    best, out = ks.select_model(table=tab)
    assert best == 1 and out is tab and ks.model is ks.candidates[1]
    best, _ = ks.select_model("unscaled_euclid_mean", tab)
    assert best == 1


def test_select_model_averages_per_output_metrics_over_trials_and_outputs():
    ks = _bare()
    tab = _table([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
    tab["rmse"] = np.array([[[0.1, 0.9], [0.1, 0.9]], [[0.4, 0.4], [0.4, 0.5]], [[0.2, 0.2], [0.9, 0.9]]])   # 0.5, 0.425, 0.55
    best, _ = ks.select_model("rmse", tab)
    assert best == 1 and ks.model is ks.candidates[1]
    tab["nrmse"] = tab["rmse"][::-1].copy()
    assert ks.select_model("nrmse", tab)[0] == 1
    tab["mean"][2] = 0.01
    assert ks.select_model("mean", tab)[0] == 2 and ks.model is ks.candidates[2]


def test_select_model_ranks_nan_and_diverged_candidates_last():
    ks = _bare()
    tab = _table([[np.nan, 0.0], [0.7, 0.9], [0.01, 0.01]], diverged=[[False, False], [False, False], [False, True]])
    best, _ = ks.select_model(table=tab)                          # 0: NaN; 2: least, but diverged on one trial
    assert best == 1 and ks.model is ks.candidates[1]
    tab = _table([[np.inf, 0.1], [0.7, 0.9], [0.8, 0.9]])
    assert ks.select_model(table=tab)[0] == 1
    # a per-output NaN (nrmse of a constant output) removes the candidate for that metric only
    tab = _table([[0.1, 0.1], [0.7, 0.9], [0.8, 0.9]])
    tab["nrmse"][0, 1, 0] = np.nan
    assert ks.select_model("nrmse", tab)[0] == 1 and ks.select_model("euclid_mean", tab)[0] == 0


def test_select_model_raises_when_every_candidate_diverged():
    ks = _bare()
    before = ks.model
    tab = _table([[np.nan, 1.0], [np.inf, 1.0], [0.1, 0.2]], diverged=[[True, False], [True, False], [False, True]])
    with pytest.raises(ValueError, match="diverged"):
        ks.select_model(table=tab)
    assert ks.model is before


def test_select_model_checks_its_arguments_and_accepts_a_single_candidate():
    ks = _bare()
    with pytest.raises(ValueError, match="metric"):
        ks.select_model("euclid", _table([[0.1], [0.2], [0.3]]))
    with pytest.raises(ValueError, match="candidates"):
        ks.select_model(table=_table([[0.1], [0.2]]))
    one = _bare(single=True)
    best, _ = one.select_model(table=_table([[0.1, 0.4]]))
    assert best == 0 and one.model is one.candidates


def _with_valdata(single=False):
    ks = _bare(single=single)
    rng = np.random.default_rng(0)
    ks.params = {"n": 2, "m": 1, "nd": 0, "nw": 0, "scale": {"y_factor": np.array([2.0, 0.5]), "y_offset": np.array([1.0, -1.0])}}
    ks.loaded, ks.model_type, ks.time_type = False, "linear", "discrete"
    ks.valdata = [{"t": 0.1 * np.arange(T), "y": rng.uniform(-1, 1, (T, 2)), "u": rng.uniform(-1, 1, (T, 1))} for T in (5, 3)]
    calls = []

    def stub(models=None, valdata=None, want_sim=False):
        calls.append((models, valdata, want_sim))
        sim = [[v["y"] + 0.25 * (q + 1) for q, v in enumerate(valdata)]]
        tab = _table([[10.0 + q for q in range(len(valdata))]])
        tab["sim"] = sim
        return tab

    ks.val_candidates = stub
    return ks, calls


def test_valnplot_model_chooses_the_candidate_as_the_reference_does():
    ks, calls = _with_valdata()
    ks.valNplot_model()                                           # no id: the first of the list (Ksysid.m:1942-1943)
    ks.valNplot_model(2)
    ks.valNplot_model(model_id=0)
    assert [c[0] for c in calls] == [ks.candidates[0], ks.candidates[2], ks.candidates[0]]
    assert all(c[0] is m for c, m in zip(calls, (ks.candidates[0], ks.candidates[2], ks.candidates[0])))
    assert all(c[1] is ks.valdata and c[2] is True for c in calls)
    for bad in (3, -1, 1.5):
        with pytest.raises(IndexError):
            ks.valNplot_model(bad)
    one, calls1 = _with_valdata(single=True)
    one.valNplot_model()                                          # a single candidate is not a list (:1939-1941, :1944-1945)
    one.valNplot_model(None)
    assert all(c[0] is one.candidates for c in calls1) and len(calls1) == 2
    with pytest.raises(IndexError):
        one.valNplot_model(1)
    none = _bare()
    none.candidates = None
    with pytest.raises(ValueError, match="train_models"):
        none.valNplot_model()


def test_valnplot_model_refuses_plots_and_the_save_dialog():
    ks, calls = _with_valdata()
    with pytest.raises(NotImplementedError):
        ks.valNplot_model(None, False, True)
    with pytest.raises(NotImplementedError):
        ks.valNplot_model(None, True)
    with pytest.raises(NotImplementedError):
        ks.valNplot_model(plot_on=True)
    assert calls == []


def test_valnplot_model_returns_the_dicts_of_val_model_and_get_error():
    ks, _ = _with_valdata()
    results, err = ks.valNplot_model(1)
    assert len(results) == len(err) == 2
    for q, (res, e, v) in enumerate(zip(results, err, ks.valdata)):
        assert set(res) == {"t", "sim", "real", "error"} and res["error"] is e
        assert np.array_equal(res["t"], v["t"]) and np.array_equal(res["real"]["y"], v["y"]) and np.array_equal(res["sim"]["u"], v["u"])
        assert np.array_equal(res["sim"]["y"], v["y"] + 0.25 * (q + 1))
        d = 0.25 * (q + 1)
        # abs / euclid come from the returned trajectory, the reduced metrics from the table
        np.testing.assert_allclose(e["abs"], np.full(v["y"].shape, d), atol=1e-15)
        np.testing.assert_allclose(e["euclid"], np.full(len(v["t"]), d * np.sqrt(2.0)), atol=1e-15)
        np.testing.assert_allclose(e["unscaled"]["euclid"], np.full(len(v["t"]), d * np.sqrt(4.0 + 0.25)), atol=1e-15)
        assert e["euclid_mean"] == 10.0 + q and e["unscaled"]["euclid_mean"] == 3.0 * (10.0 + q)
        assert np.array_equal(e["mean"], np.full(2, 10.0 + q)) and np.array_equal(e["rmse"], e["nrmse"])
        assert set(e) == {"abs", "mean", "rmse", "nrmse", "euclid", "euclid_mean", "unscaled"}
