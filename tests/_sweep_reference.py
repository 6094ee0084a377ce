"""Test-side reference of the random-system sweep (evaluate_rand_models.m:47-143) for ARBITRARY degree-ordered exponent
tables, beyond the 1-state / 1-input systems of the benchmark: a generator of small systems, the pipeline scale -> snapshot
pairs -> lift -> least squares -> model -> validation rollout -> normalised mean error (through oracle/koopman_oracle.py for
full tables, restated in plain numpy for sparse ones), and a validation rollout of a GIVEN model in np.longdouble, which
isolates the device's rollout kernels from its fit.  Shared by tests/test_sweep_reference.py (CPU) and
tests/test_gpu_sweep_shapes.py; not collected by pytest."""
import functools

import numpy as np

from oracle import koopman_oracle as ko

EPS = 2.2e-16
NB, K_TRIALS, T_TRAIN, T_VAL = 3, 3, 60, 40          # 3 (T - 1) - 1 = 176 pairs: one full 128-pair tile and a ragged one


def _rows(nv, *monos):
    """Exponent rows over nv variables from tuples of (variable, exponent) pairs."""
    e = np.zeros((len(monos), nv), dtype=np.int64)
    for r, mono in enumerate(monos):
        for v, p in mono:
            e[r, v] = p
    return e


def _full(nv, D):
    return ko.poly_exponents(nv, D)[nv:]


# name -> (model type, n, m, exponent rows beyond the variables themselves, expected kp_timer_get(14) code of the nested call).
# Dictionary variables: the n states; for nonlinear models [states; inputs].  The code is 1000 G + 100 F + 10 U + R
# (include/koopman_hip.h).  E of the issue's table (bilinear, n = m = 3, xyz) would have N = 5 and W = 20 > 16; a three-factor
# monomial needs n >= 3, hence N >= 5 and m <= 2: E1 is that shape (W = 15), E2 the full 16-wide tile with m = 3 (no monomial).
CASES = {
    "A": ("linear", 2, 2, _full(2, 3), 4201),
    "B": ("linear", 3, 3, _rows(3, ((0, 1), (1, 1)), ((1, 1), (2, 1)), ((0, 1), (1, 1), (2, 1))), 4301),
    "C": ("linear", 4, 1, _rows(4, ((0, 2),), ((0, 1), (1, 1), (2, 1), (3, 1))), 4401),
    "D": ("bilinear", 2, 1, _full(2, 2), 4211),
    "E1": ("bilinear", 3, 2, _rows(3, ((0, 1), (1, 1), (2, 1))), 4311),
    "E2": ("bilinear", 3, 3, _rows(3), 4111),
    "F": ("bilinear", 4, 1, _rows(4, ((0, 1), (1, 1), (2, 1), (3, 1))), 4411),
    "G": ("bilinear", 1, 1, _rows(1, ((0, 9),)), 4201),
    "H": ("bilinear", 4, 1, _rows(4, ((0, 2),), ((0, 1), (1, 1), (2, 1), (3, 1))), 4501),
    "I": ("nonlinear", 2, 2, _full(4, 2), 4201),
    "J": ("nonlinear", 2, 3, _rows(5), 1001),
    "K": ("nonlinear", 4, 1, _rows(5), 1001),
    "L": ("linear", 5, 1, _rows(5), 1002),
    "M": ("bilinear", 7, 1, _rows(7), 1002),
    "N": ("nonlinear", 5, 3, _rows(8), 1002),
    "O": ("linear", 1, 1, _rows(1, ((0, 13),)), 3101),
    "P": ("bilinear", 1, 1, _rows(1, ((0, 6),)), 3111),
    "Q": ("nonlinear", 1, 1, _rows(2, ((0, 4),), ((0, 3), (1, 1))), 3201),
    "R": ("bilinear", 1, 1, _rows(1), 4111),
    "LASSO": ("nonlinear", 2, 1, _full(3, 2), 4201),
}
FLAT_CODE = 5003                                     # kp_sweep_eval: kp_small_fit_kernel with recipes, kp_sweep_rollout_kernel


def case_dims(name):
    """(model type, n, m, nv, exponent rows, top degree, N, W, code) of a case."""
    mt, n, m, ex, code = CASES[name]
    nv = n + (m if mt == "nonlinear" else 0)
    assert ex.shape[1] == nv
    D = int(ex.sum(axis=1).max()) if ex.shape[0] else 1
    N = nv + ex.shape[0] + 1
    W = N + m if mt == "linear" else N * (m + 1) if mt == "bilinear" else N
    return mt, n, m, nv, ex, D, N, W, code


def is_full(ex, nv, D):
    f = _full(nv, D)
    return f.shape == ex.shape and bool((f == ex).all())


def rows_of_degree(ex, j):
    """Rows of the table that the degree-j dictionary keeps (the variables and the constant are always in)."""
    return ex[ex.sum(axis=1) <= j]


def width(mt, m, N):
    return N + m if mt == "linear" else N * (m + 1) if mt == "bilinear" else N


# ------------------------------------------------------------------------------------------------------------------------
# systems
# ------------------------------------------------------------------------------------------------------------------------
def make_systems(n, m, nb=NB, k=K_TRIALS, T=T_TRAIN, Tv=T_VAL, seed=0):
    """nb systems y+ = A y + B u + 0.05 tanh(y * u_0) with rho(A) = 0.8, B = 0.2 randn, inputs uniform in [-1, 1]; k training
    trials of T rows and one validation trial of Tv rows each, as the data4sysid structs that sweep._stack_raw takes.  The
    validation trial is redrawn until its outputs stay inside the range of the training outputs: scaled by the training range
    they then lie in [-1, 1], where no monomial extrapolates (a validation output of 1.35 makes x^13 = 49 and the degree-13
    model of such a system leaves the region it was fitted on: its error is 18, not 0.05, and every rounding is amplified)."""
    rng = np.random.default_rng(seed)
    systems = []
    for _ in range(nb):
        A = rng.standard_normal((n, n))
        A *= 0.8 / np.abs(np.linalg.eigvals(A)).max()
        B = 0.2 * rng.standard_normal((n, m))
        def trial(rows):
            u = rng.uniform(-1, 1, (rows, m)); y = np.zeros((rows, n)); y[0] = rng.uniform(-0.5, 0.5, n)
            for t in range(rows - 1):
                y[t + 1] = A @ y[t] + B @ u[t] + 0.05 * np.tanh(y[t] * u[t, 0])
            return {"t": np.arange(rows) * 0.01, "y": y, "u": u}
        trials = [trial(T) for _ in range(k)]
        lo, hi = np.min([tr["y"].min(axis=0) for tr in trials], axis=0), np.max([tr["y"].max(axis=0) for tr in trials], axis=0)
        for _ in range(10000):                       # see the docstring: the first validation trial inside the training range
            v = trial(Tv)
            if (v["y"] >= lo).all() and (v["y"] <= hi).all():
                break
        else:
            raise RuntimeError("make_systems: no validation trial inside the training range")
        trials.append(v)
        systems.append({"train": trials[:k], "val": trials[k:]})
    return systems


def zero_system(like):
    """A system of the same layout whose outputs and inputs are all zero (its Gram matrix is singular)."""
    z = lambda tr: {"t": tr["t"].copy(), "y": np.zeros_like(tr["y"]), "u": np.zeros_like(tr["u"])}
    return {"train": [z(tr) for tr in like["train"]], "val": [z(tr) for tr in like["val"]]}


def prepare(system):
    """Scaled snapshot pairs (all, in time order) and the validation trial scaled with the training data's factors."""
    sd, sc = ko.get_scale(ko.merge_trials(system["train"]))
    pairs = ko.snapshot_pairs(sd, 0)
    v = system["val"][0]
    val = {"t": v["t"], "y": ko.scaledown(sc, "y", v["y"]), "u": ko.scaledown(sc, "u", v["u"])}
    return pairs, val


# ------------------------------------------------------------------------------------------------------------------------
# plain restatement: lift, least squares, model, rollout, error
# ------------------------------------------------------------------------------------------------------------------------
def lift(V, ex):
    """[V, prod_v V_v^e_v for every row e of ex, 1] by repeated multiplication, in V's number type."""
    V = np.atleast_2d(V)
    cols = [V]
    for e in ex:
        c = np.ones(V.shape[0], dtype=V.dtype)
        for v, p in enumerate(e):
            for _ in range(int(p)):
                c = c * V[:, v]
        cols.append(c[:, None])
    cols.append(np.ones((V.shape[0], 1), dtype=V.dtype))
    return np.hstack(cols)


def px_py(mt, ex, pairs):
    a, b, u = pairs["alpha"], pairs["beta"], pairs["u"]
    if mt == "nonlinear":
        return lift(np.hstack([a, u]), ex), lift(np.hstack([b, u]), ex)
    px, py = lift(a, ex), lift(b, ex)
    if mt == "bilinear":
        return (np.hstack([px] + [px * u[:, [i]] for i in range(u.shape[1])]),
                np.hstack([py] + [py * u[:, [i]] for i in range(u.shape[1])]))
    return np.hstack([px, u]), np.hstack([py, u])


def project_linear(K, N, Px, Py, u):
    """get_model's M-projection (Ksysid.m:1206-1225) by lstsq: returns M A, M B and cond(L)."""
    UT = K.T
    A, B = UT[:N, :N], UT[:N, N:]
    L = Px[:, :N] @ A.T + u @ B.T
    M = np.linalg.lstsq(L, Py[:, :N], rcond=None)[0].T
    return M @ A, M @ B, float(np.linalg.cond(L))


def model_of(mt, n, m, K, N, Px=None, Py=None, u=None):
    """What the validation rollout needs of K: ('linear', MA, MB) | ('bilinear', A, B) | ('nonlinear', Kf)."""
    if mt == "linear":
        A, B, _ = project_linear(K, N, Px, Py, u)
        return ("linear", A, B)
    UT = K.T
    if mt == "bilinear":
        return ("bilinear", UT[:N, :N], UT[:N, N:])
    return ("nonlinear", K[:, :n].T)


def rollout_error(model, n, m, ex, val, dtype=np.float64):
    """Validation rollout of `model` from the first validation row, the inputs as recorded, and
    err_j = mean_t |sim - real|_j / mean_t |real|_j (evaluate_rand_models.m:70-72; the first simulated row is the measured one,
    Ksysid.m:1654), everything in `dtype`."""
    y = np.asarray(val["y"], dtype=dtype); u = np.asarray(val["u"], dtype=dtype)
    Tv = y.shape[0]
    sim = np.zeros((Tv, n), dtype=dtype); sim[0] = y[0]
    mats = [np.asarray(a, dtype=dtype) for a in model[1:]]
    if model[0] == "nonlinear":
        zeta = y[0].copy()
        for t in range(Tv - 1):
            zeta = mats[0] @ lift(np.concatenate([zeta, u[t]])[None, :], ex)[0]
            sim[t + 1] = zeta
    else:
        z = lift(y[0][None, :], ex)[0]
        N = z.shape[0]
        for t in range(Tv - 1):
            if model[0] == "linear":
                z = mats[0] @ z + mats[1] @ u[t]
            else:
                Au = mats[0].copy()
                for i in range(m):
                    Au = Au + u[t, i] * mats[1][:, i * N:(i + 1) * N]
                z = Au @ z
            sim[t + 1] = z[:n]
    err = (np.abs(sim - y).sum(axis=0) / Tv) / (np.abs(y).sum(axis=0) / Tv)
    return np.asarray(err, dtype=np.float64)


def sparse_pipeline(mt, n, m, ex, pairs, val):
    """One (system, degree) of the sweep for the exponent rows `ex`: K, err (n), cond(L) (linear models, else None), G, C."""
    Px, Py = px_py(mt, ex, pairs)
    K = np.linalg.lstsq(Px, Py, rcond=None)[0]
    N = ex.shape[1] + ex.shape[0] + 1
    condL = project_linear(K, N, Px, Py, pairs["u"])[2] if mt == "linear" else None
    model = model_of(mt, n, m, K, N, Px, Py, pairs["u"])
    return {"K": K, "err": rollout_error(model, n, m, ex, val), "condL": condL, "G": Px.T @ Px, "C": Px.T @ Py}


def oracle_pipeline(mt, n, m, j, pairs, val):
    """The same through oracle/koopman_oracle.py for the full degree-j table."""
    dic = ko.build_dictionary(mt, n, m, ["poly"], [j])
    koop = ko.get_koopman(dic, pairs)
    mdl = {"linear": ko.get_model, "bilinear": ko.get_blmodel, "nonlinear": ko.get_nlmodel}[mt](dic, koop, n)
    r = ko.val_model(dic, mdl, val, 0)
    e = ko.get_error(r["sim_y"], r["real_y"])
    err = e["mean"] / (np.abs(r["real_y"]).sum(axis=0) / r["real_y"].shape[0])
    condL = None
    if mt == "linear":
        condL = float(np.linalg.cond(koop["Px"] @ mdl["A_raw"].T + koop["u"] @ mdl["B_raw"].T))
    Px, Py = ko.px_py(dic, pairs)
    G, C = ko.gram(Px, Py)
    return {"K": koop["K"], "err": np.asarray(err, dtype=np.float64), "condL": condL, "G": G, "C": C}


def reference(mt, n, m, ex, D, systems):
    """Every degree 1..D of every system: ref[dj][i] = dict(K, err, condL, G, C, ex) - the oracle for full tables, the
    restatement for sparse ones."""
    nv = ex.shape[1]
    full = is_full(ex, nv, D)
    prepared = [prepare(s) for s in systems]
    out = []
    for j in range(1, D + 1):
        exj = rows_of_degree(ex, j)
        row = []
        for pairs, val in prepared:
            r = oracle_pipeline(mt, n, m, j, pairs, val) if full else sparse_pipeline(mt, n, m, exj, pairs, val)
            r["ex"] = exj
            row.append(r)
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def case_systems(name, k=K_TRIALS, T=T_TRAIN, Tv=T_VAL):
    """The systems of a case (seeded by its name), computed once; callers must not modify them."""
    mt, n, m = CASES[name][:3]
    return tuple(make_systems(n, m, NB, k, T, Tv, seed=100 + sorted(CASES).index(name)))


@functools.lru_cache(maxsize=None)
def case_reference(name, k=K_TRIALS, T=T_TRAIN, Tv=T_VAL):
    """reference() of a case's systems, computed once and shared; callers must not modify it."""
    mt, n, m, nv, ex, D, N, W, code = case_dims(name)
    return reference(mt, n, m, ex, D, list(case_systems(name, k, T, Tv)))


# ------------------------------------------------------------------------------------------------------------------------
# tolerances (the issue's section 4)
# ------------------------------------------------------------------------------------------------------------------------
def rollout_floor(Tv):
    """(d), bilinear and nonlinear: each step sums at most 16 (m + 1) products into each of 16 components and the systems
    contract, so the per-step rounding adds over Tv steps; 4 for the two divisions and the absolute-value sums."""
    return 4 * 16 * Tv * EPS


def linear_rollout_tol(condL):
    """(d), linear: the device projects by normal equations on L (the rule of test_fit_arm_data_matches_oracle_lstsq)."""
    return max(1e-9, 50 * condL ** 2 * EPS)


def rollout_reference_ld(mt, n, m, exj, K, pairs, val):
    """err of the long-double validation rollout of the model that K (as the device returned it) defines; for linear models
    A, B come from K by the reference projection."""
    Px = Py = None
    if mt == "linear":
        Px, Py = px_py(mt, exj, pairs)
    N = exj.shape[1] + exj.shape[0] + 1
    return rollout_error(model_of(mt, n, m, K, N, Px, Py, pairs["u"]), n, m, exj, val, dtype=np.longdouble)
