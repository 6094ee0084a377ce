"""GPU tests of kp_nmpc_simulate (Nmpc.simulate, Kmpc.run_simulations of a nonlinear controller): whole closed loops of
the nonlinear MPC with the identified model as the plant, one workgroup per trial, one launch.

Models: the first three of test_small_random_models_match_host_restatement (its costs, box +-0.8, slope 0.3, starts drawn
as it draws them; reference 0.4 sin(0.5 k) on output 1, 13 rows) and the arm's controller with the slope rows (first 13
rows of the block-M, the stored start), all at options (300, 1e-11, 1e-10).  The `loops` fixture runs each loop once and
replays EVERY recorded step with the single-step kernel, Nmpc.step(Y[k-1], U[k-1], window); it asserts that every replayed
step returns KP_OK, so no step is left out of any comparison below.

Teacher-forced parity: the replay's row 2 is U[k] to 1e-8 (the bound test_gpu_nmpc.py holds two routes to one optimum to at
these options), its row 1 is U[k-1] bit for bit, its z_1 and the oracle's Kf econ_full([Y[k-1]; U[k-1]]) are Y[k] to
1e-12 max(1, |Y|), and the step's status in `info` is the replay's.

Free-running runs on the arm (20 steps of the block-M, Kmpc at nmpc_tol 1e-10, 300 iterations) are compared in scaled
units.  Two correct closed loops drift apart by what their SQPs leave of the optimum, fed back through the plant; that
noise is MEASURED in the `free_run` fixture between two host loops (Kmpc.run_simulation) through the single-step kernel,
one cold-started, one warm-started, and the device loops have to stay within 10 times it of the cold host loop.
Measured on an MI355X: noise 9.3e-12, so the bound is 9.3e-11; the cold device loop and run_simulations differ from the
cold host loop by 3.2e-14, the warm device loop by 9.3e-12.  The fixture measures and prints the noise on
every run."""
import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from test_gpu_fit import make_basis
from test_gpu_mpc_sim import SIM_PINNED_BYTES, copies_of, sim_block_bytes
from test_gpu_nmpc import arm_ks, arm_nl, arm_nmpc, arm_setup, example_kmpc, synth  # noqa: F401  (fixtures among them)
from test_nmpc_host import load_nmpc_golden

pytestmark = pytest.mark.gpu

OPTIONS = (300, 1e-11, 1e-10)
NREF = 13
SMALL = [(2, 1, 8, ["poly"], [3]), (3, 2, 6, ["hermite"], [2]), (2, 2, 5, ["gaussian"], [5])]
SMALL_IDS = ["poly3", "hermite2", "gaussian5"]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def small_model(ctx, nz, m, Np, obs, deg):
    """The model, controller and start of test_small_random_models_match_host_restatement (same seeds, same draws)."""
    pairs = synth(nz, m, Ns=600, seed=3 * nz + m)
    rng = np.random.default_rng(nz * 10 + m)
    centres = [rng.uniform(-1, 1, (nz + m, d)) for o, d in zip(obs, deg) if o == "gaussian"]
    dic = ko.build_dictionary("nonlinear", nz, m, obs, deg, pairs, dim_red=False, gaussian_centres=centres or None)
    Kf = ko.get_nlmodel(dic, ko.get_koopman(dic, pairs), nz)["Kf"]
    dev = kra.Nmpc(ctx, make_basis(ctx, dic), Kf, Np, np.eye(nz)[:1], 5.0, 50.0, np.full(m, 0.05), -0.8 * np.ones(m),
                   0.8 * np.ones(m), 0.3, None)
    dev.set_options(*OPTIONS)
    zeta = rng.uniform(-0.5, 0.5, nz); up = rng.uniform(-0.3, 0.3, m)
    ref = (0.4 * np.sin(0.5 * np.arange(NREF)))[:, None]
    return {"dic": dic, "Kf": Kf, "dev": dev, "ref": ref, "y0": zeta, "u0": up, "Np": Np, "rng": rng}


def window(ref, k, Np):
    """Rows k-1 .. k-1+Np of the reference, its last row repeated behind its end (Kmpc._pad_ref), vectorised."""
    idx = np.minimum(np.arange(k - 1, k + Np), len(ref) - 1)
    return ref[idx].ravel()


def replay(c, U, Y, info, steps):
    """Replays steps 1 .. steps of one recorded trial with the single-step kernel and makes the teacher-forced checks.
    Returns the replayed Z of every step."""
    dev, dic, Kf, ref, Np = c["dev"], c["dic"], c["Kf"], c["ref"], c["Np"]
    Zs = []
    for k in range(1, steps + 1):
        Us, Z, inf, st = dev.step(Y[k - 1], U[k - 1], window(ref, k, Np))
        assert st == F.KP_OK, (k, st, inf)                          # the condition: every step of the step kernel converges
        assert np.abs(Us[1] - U[k]).max() <= 1e-8, (k, np.abs(Us[1] - U[k]).max())
        assert same_bits(Us[0], U[k - 1]), k
        tol = 1e-12 * max(1.0, np.abs(Y[k]).max())
        assert np.abs(Z[1] - Y[k]).max() <= tol, (k, np.abs(Z[1] - Y[k]).max())
        yo = Kf @ ko.econ_full(dic, np.concatenate([Y[k - 1], U[k - 1]])[None, :])[0]
        assert np.abs(yo - Y[k]).max() <= tol, (k, np.abs(yo - Y[k]).max())
        assert info[k - 1, 2] == st, (k, info[k - 1])
        Zs.append(Z)
    return np.array(Zs)


@pytest.fixture(scope="module")
def arm_case(ctx, arm_setup):
    dic, mdl, sc, basis, ref_sc = arm_setup
    d = load_nmpc_golden()
    dev, _ = arm_nmpc(ctx, arm_setup)
    dev.set_options(*OPTIONS)
    return {"dic": dic, "Kf": mdl["Kf"], "dev": dev, "ref": ref_sc[:NREF], "y0": ko.scaledown(sc, "y", d["Y"][0]),
            "u0": ko.scaledown(sc, "u", d["U"][0]), "Np": 10, "ref_all": ref_sc, "sc": sc}


@pytest.fixture(scope="module")
def loops(ctx, arm_case):
    """Every model's cold loop of NREF - 1 steps, run once and replayed step by step (the teacher-forced checks and the
    condition that every step converges are made here, once, for all tests that use the recorded loops)."""
    out = {}
    cases = dict(zip(SMALL_IDS, [small_model(ctx, *p) for p in SMALL]))
    cases["arm"] = arm_case
    for name, c in cases.items():
        U, Y, info, sd, st = c["dev"].simulate(c["ref"], c["y0"][None], c["u0"][None])
        print(f"{name}: status {st[0]}, steps {sd[0]}, SQP iterations {info[0, :, 0].astype(int).tolist()}, "
              f"KKT max {info[0, :, 1].max():.1e}, |y| max {np.abs(Y[0]).max():.3f}")
        assert st[0] == F.KP_OK and sd[0] == NREF - 1, (name, st, sd, info[0])
        assert same_bits(U[0, 0], c["u0"]) and same_bits(Y[0, 0], c["y0"])
        assert np.isfinite(U).all() and np.isfinite(Y).all() and np.isfinite(info).all()
        Z = replay(c, U[0], Y[0], info[0], NREF - 1)
        out[name] = dict(c, U=U[0], Y=Y[0], info=info[0], Z=Z)
    return out


# ---- 1. teacher-forced parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL_IDS + ["arm"])
def test_teacher_forced_parity(loops, name):
    r = loops[name]                          # (the checks themselves: replay(), run by the fixture on every step)
    assert r["Z"].shape == (NREF - 1, r["Np"] + 1, r["Y"].shape[1])
    assert (r["info"][:, 2] == F.KP_OK).all() and (r["info"][:, 0] >= 1).all()
    if name != "arm":                        # the applied inputs keep the box and the slope limit
        dU = np.abs(np.diff(r["U"], axis=0))
        assert (np.abs(r["U"]) <= 0.8 + 1e-9).all() and (dU <= 0.3 + 1e-9).all()


# ---- 2. free-running against the host loop -----------------------------------------------------------------------------
FREE_ROWS = 21


@pytest.fixture(scope="module")
def free_run(arm_ks, golden):
    """The host loop run_simulation on the arm's nonlinear controller, cold- and warm-started: two routes through the
    single-step kernel to the same optima.  Their difference in scaled units is the yardstick (bound = 10 x noise)."""
    ks = arm_ks
    ref = golden["blockM_ref"]["y"][:FREE_ROWS]
    y0 = load_nmpc_golden()["Y"][0]
    kw = dict(nmpc_tol=1e-10, nmpc_max_iter=300)
    cold, warm = example_kmpc(ks, **kw), example_kmpc(ks, nmpc_warm_start=True, **kw)
    hc = cold.run_simulation(ref, y0, np.zeros(3))
    hw = warm.run_simulation(ref, y0, np.zeros(3))
    assert hc["Y"].shape == hw["Y"].shape == (FREE_ROWS, 6)
    sy, su = ks.scaledown_y, ks.scaledown_u
    noise = max(np.abs(sy(hc["Y"]) - sy(hw["Y"])).max(), np.abs(su(hc["U"]) - su(hw["U"])).max())
    print("free-running noise (host loop cold vs warm, %d steps, scaled units): %.3e; bound %.3e; statuses cold %s warm %s"
          % (FREE_ROWS - 1, noise, 10 * noise, np.unique(hc["nmpc_info"][:, 2]), np.unique(hw["nmpc_info"][:, 2])))
    assert noise > 0.0
    return {"ref": ref, "y0": y0, "cold": cold, "warm": warm, "host": hc, "noise": noise, "bound": 10.0 * noise}


def scaled_diff(ks, a, b):
    return max(np.abs(ks.scaledown_y(a["Y"]) - ks.scaledown_y(b["Y"])).max(),
               np.abs(ks.scaledown_u(a["U"]) - ks.scaledown_u(b["U"])).max())


def test_free_running_matches_the_host_loop(arm_ks, free_run):
    ks, host = arm_ks, free_run["host"]
    ref, y0 = free_run["ref"], free_run["y0"]
    res = free_run["cold"].run_simulations([ref], y0[None], np.zeros((1, 3)))
    assert len(res) == 1
    dev = res[0]
    assert set(dev) == set(host) | {"steps_done"} and dev["steps_done"] == FREE_ROWS - 1
    for k in ("T", "U", "Y", "K", "R", "Z", "comp_time", "nmpc_info"):
        assert dev[k].shape == host[k].shape, (k, dev[k].shape, host[k].shape)
    assert (dev["K"] == host["K"]).all() and np.abs(dev["T"] - host["T"]).max() < 1e-12
    assert np.abs(dev["R"] - host["R"]).max() < 1e-12
    assert (dev["comp_time"] > 0).all() and np.ptp(dev["comp_time"]) == 0
    d_rs = scaled_diff(ks, dev, host)
    # the device loop itself, cold and warm, in scaled units
    mpc = free_run["cold"]
    ysc, y0s, u0s = mpc.scaledown_ref(ref), ks.scaledown_y(y0)[None], ks.scaledown_u(np.zeros(3))[None]
    hY, hU = ks.scaledown_y(host["Y"]), ks.scaledown_u(host["U"])
    d = {}
    for warm in (False, True):
        U, Y, info, sd, st = mpc.dev.simulate(ysc, y0s, u0s, warm=warm)
        assert sd[0] == FREE_ROWS - 1 and st[0] != F.KP_ERR_QP_FAIL
        d[warm] = max(np.abs(Y[0] - hY).max(), np.abs(U[0] - hU).max())
    print("vs the cold host loop: device cold %.3e, device warm %.3e, run_simulations %.3e (noise %.3e, bound %.3e)"
          % (d[False], d[True], d_rs, free_run["noise"], free_run["bound"]))
    assert d[False] <= free_run["bound"] and d[True] <= free_run["bound"] and d_rs <= free_run["bound"]
    # a warm-started controller goes through the warm device loop, and its warm start does not leak into the next run
    rw = free_run["warm"].run_simulations([ref], y0[None], None)[0]
    assert scaled_diff(ks, rw, host) <= free_run["bound"]
    h2 = free_run["warm"].run_simulation(ref[:4], y0, np.zeros(3))
    h3 = free_run["warm"].run_simulation(ref[:4], y0, np.zeros(3))
    assert same_bits(h2["U"], h3["U"]) and same_bits(h2["Y"], h3["Y"])


# ---- 3. batch independence, bit for bit ---------------------------------------------------------------------------------
SHIFTS = (0, 3, 9, 20, 27)


def test_a_trial_does_not_depend_on_the_batch_it_runs_in(arm_case):
    dev = arm_case["dev"]
    rng = np.random.default_rng(3)
    nb = 5
    ref = np.stack([arm_case["ref_all"][i:i + NREF] for i in SHIFTS])
    d, sc = load_nmpc_golden(), arm_case["sc"]            # the stored run's state at the first row of each reference, perturbed
    y0 = ko.scaledown(sc, "y", d["Y"][list(SHIFTS)]) + 0.01 * rng.standard_normal((nb, 6))
    u0 = ko.scaledown(sc, "u", d["U"][list(SHIFTS)]) + 0.02 * rng.standard_normal((nb, 3))
    for warm in (False, True):
        U, Y, info, sd, st = dev.simulate(ref, y0, u0, warm=warm)
        assert (st != F.KP_ERR_QP_FAIL).all() and (sd == NREF - 1).all()
        for i in range(nb):
            U1, Y1, i1, sd1, st1 = dev.simulate(ref[i:i + 1], y0[i:i + 1], u0[i:i + 1], warm=warm)
            assert same_bits(U1[0], U[i]) and same_bits(Y1[0], Y[i]) and same_bits(i1[0], info[i]), (warm, i)
            assert sd1[0] == sd[i] and st1[0] == st[i]
    # one reference for all trials = the same reference repeated per trial
    Us, Ys, is_, sds, sts = dev.simulate(ref[1], y0, u0)
    Ur, Yr, ir, sdr, str_ = dev.simulate(np.stack([ref[1]] * nb), y0, u0)
    assert same_bits(Us, Ur) and same_bits(Ys, Yr) and same_bits(is_, ir) and (sds == sdr).all() and (sts == str_).all()
    assert not same_bits(Us[0], Us[1])


def test_more_trials_than_are_resident(ctx):
    c = small_model(ctx, *SMALL[0])
    dev, rng = c["dev"], c["rng"]
    nb = 300
    y0 = rng.uniform(-0.5, 0.5, (10, 2)); u0 = rng.uniform(-0.3, 0.3, (10, 1))
    idx = np.arange(nb) % 10
    U, Y, info, sd, st = dev.simulate(c["ref"], y0[idx], u0[idx])
    assert (st != F.KP_ERR_QP_FAIL).all() and (sd == NREF - 1).all()
    for j in range(10):
        U1, Y1, i1, _, st1 = dev.simulate(c["ref"], y0[j:j + 1], u0[j:j + 1])
        rows = np.nonzero(idx == j)[0]
        assert len(rows) == 30
        assert all(same_bits(U[i], U1[0]) and same_bits(Y[i], Y1[0]) and same_bits(info[i], i1[0]) and st[i] == st1[0]
                   for i in rows), j
    assert not same_bits(Y[0], Y[1])


def test_results_copied_straight_to_the_callers_arrays(ctx):
    """A call above SIM_PINNED_BYTES copies each output straight into the caller's array; every trial of it has the bits of
    the same start run alone, which comes back through the page-locked scratch."""
    c = small_model(ctx, *SMALL[0])
    dev, rng = c["dev"], c["rng"]
    nref, nd = 5, 10
    size = lambda nb: sim_block_bytes(nb, nref, 1, 2, 1, 3, True)
    nb = nd * (SIM_PINNED_BYTES // (size(nd) - size(0)) + 1)
    assert size(nb) > SIM_PINNED_BYTES >= size(nb - 2 * nd) and size(1) <= SIM_PINNED_BYTES, (nb, size(nb))
    y0 = rng.uniform(-0.5, 0.5, (nd, 2)); u0 = rng.uniform(-0.3, 0.3, (nd, 1))
    idx = np.arange(nb) % nd
    U, Y, info, sd, st = dev.simulate(c["ref"][:nref], y0[idx], u0[idx])
    assert (st != F.KP_ERR_QP_FAIL).all() and (sd == nref - 1).all()
    for j in range(nd):
        U1, Y1, i1, sd1, st1 = dev.simulate(c["ref"][:nref], y0[j:j + 1], u0[j:j + 1])
        rows = np.nonzero(idx == j)[0]
        assert len(rows) == nb // nd
        assert copies_of(U, U1, rows) and copies_of(Y, Y1, rows) and copies_of(info, i1, rows), j
        assert copies_of(sd, sd1, rows) and copies_of(st, st1, rows), j
    assert not same_bits(Y[0], Y[1])


# ---- 4. failure stays local ---------------------------------------------------------------------------------------------
def test_a_failed_qp_ends_its_own_trial_only(ctx):
    c = small_model(ctx, *SMALL[1])
    dev = c["dev"]
    y0 = np.stack([c["y0"], c["y0"], c["y0"] + 0.05])
    u0 = np.stack([c["u0"], np.array([5.0, 0.0]), c["u0"] + 0.05])      # the middle one: outside the input box
    U, Y, info, sd, st = dev.simulate(c["ref"], y0, u0)
    assert st[1] == F.KP_ERR_QP_FAIL and sd[1] == 0
    assert same_bits(U[1, 0], u0[1]) and same_bits(Y[1, 0], y0[1])
    assert np.isnan(U[1, 1:]).all() and np.isnan(Y[1, 1:]).all() and np.isnan(info[1]).all()
    for i in (0, 2):
        U1, Y1, i1, sd1, st1 = dev.simulate(c["ref"], y0[i:i + 1], u0[i:i + 1])
        assert st[i] == st1[0] != F.KP_ERR_QP_FAIL and sd[i] == sd1[0] == NREF - 1
        assert same_bits(U1[0], U[i]) and same_bits(Y1[0], Y[i]) and same_bits(i1[0], info[i]), i
        assert np.isfinite(U[i]).all() and np.isfinite(Y[i]).all()


# ---- 5. unconverged steps do not end a trial ----------------------------------------------------------------------------
def test_unconverged_steps_do_not_end_a_trial(ctx):
    c = small_model(ctx, *SMALL[0])
    dev = c["dev"]
    dev.set_options(1, OPTIONS[1], OPTIONS[2])
    for warm in (False, True):
        U, Y, info, sd, st = dev.simulate(c["ref"], c["y0"][None], c["u0"][None], warm=warm)
        assert (info[0, :, 2] == F.KP_ERR_NOT_CONVERGED).all() and (info[0, :, 0] == 1).all()
        assert sd[0] == NREF - 1 and st[0] == F.KP_ERR_NOT_CONVERGED
        assert np.isfinite(U).all() and np.isfinite(Y).all() and np.isfinite(info).all()


# ---- 6. state bounds ------------------------------------------------------------------------------------------------------
def test_state_bounds_hold_along_the_loop(ctx):
    """An upper bound on the tracked state of the hermite-2 model, 0.3 of the way up the climb of the unbounded loop (from
    -0.34 to -0.21; the second input can turn that state's drift around, so the bound can be held): it binds along the run,
    and the start (z_0 and z_1 = F(z_0, u_0), which no input of the first step can move) lies inside."""
    c = small_model(ctx, *SMALL[1])
    dev = c["dev"]
    y0, u0 = c["y0"], c["u0"]
    U, Y, info, sd, st = dev.simulate(c["ref"], y0[None], u0[None])
    assert st[0] == F.KP_OK
    base = max(Y[0, 0, 0], Y[0, 1, 0])
    climb = Y[0, :, 0].max() - base
    assert climb > 0.05, Y[0, :, 0]
    lo, hi = np.full(3, -2.0), np.array([base + 0.3 * climb, 2.0, 2.0])
    dev.set_state_bounds(lo, hi)
    Ub, Yb, ib, sdb, stb = dev.simulate(c["ref"], y0[None], u0[None])
    print(f"state 1 <= {hi[0]:.4f} (unbounded loop: up to {Y[0, :, 0].max():.4f}): status {stb[0]}, steps {sdb[0]}, statuses "
          f"{ib[0, :, 2].tolist()}, iterations {ib[0, :, 0].tolist()}, KKT max {ib[0, :, 1].max():.1e}, reached {Yb[0, :, 0].max():.6f}")
    assert stb[0] == F.KP_OK and sdb[0] == NREF - 1
    Z = replay(c, Ub[0], Yb[0], ib[0], NREF - 1)
    assert (Yb[0] >= lo - 1e-8).all() and (Yb[0] <= hi + 1e-8).all()
    binding = [(np.abs(z - lo) <= 1e-7).any() or (np.abs(z - hi) <= 1e-7).any() for z in Z]
    print(f"steps with a binding state bound in their horizon: {int(np.sum(binding))} of {NREF - 1}")
    assert np.sum(binding) > 0
    assert (Z >= lo - 1e-8).all() and (Z <= hi + 1e-8).all()
    assert not same_bits(Ub, U)
    # the bounded loop in a batch with per-trial dense rows: the same bits
    U3, Y3, i3, _, _ = dev.simulate(c["ref"], np.stack([y0] * 3), np.stack([u0, u0 + 0.01, u0]))
    assert same_bits(U3[0], Ub[0]) and same_bits(U3[2], Ub[0]) and same_bits(Y3[2], Yb[0]) and same_bits(i3[0], ib[0])
    dev.set_state_bounds(None, None)
    U2, Y2, _, _, _ = dev.simulate(c["ref"], y0[None], u0[None])
    assert same_bits(U2, U) and same_bits(Y2, Y)


# ---- 7. edges and refusals ------------------------------------------------------------------------------------------------
def test_short_references_and_no_info(ctx):
    c = small_model(ctx, *SMALL[1])
    dev, ref, y0, u0 = c["dev"], c["ref"], c["y0"][None], c["u0"][None]
    U, Y, info, sd, st = dev.simulate(ref[:1], y0, u0)                    # nref = 1: no step
    assert U.shape == (1, 1, 2) and Y.shape == (1, 1, 3) and info.shape == (1, 0, 3) and sd[0] == 0 and st[0] == F.KP_OK
    assert same_bits(U[0, 0], u0[0]) and same_bits(Y[0, 0], y0[0])
    for nref in (2, 3):                                                   # one step, two steps: windows padded as _pad_ref does
        U, Y, info, sd, st = dev.simulate(ref[:nref], y0, u0)
        assert sd[0] == nref - 1 and st[0] == F.KP_OK
        replay(dict(c, ref=ref[:nref]), U[0], Y[0], info[0], nref - 1)
    Ui, Yi, ii, sdi, sti = dev.simulate(ref[:4], y0, u0)
    Un, Yn, none, sdn, stn = dev.simulate(ref[:4], y0, u0, want_info=False)
    assert none is None and same_bits(Un, Ui) and same_bits(Yn, Yi) and sdn[0] == 3 and stn[0] == sti[0]
    assert ctx.timer(F.TIMER_NMPC_SIM) > 0


def test_refusals(ctx):
    c = small_model(ctx, *SMALL[1])
    dev, ref, y0, u0 = c["dev"], c["ref"], c["y0"][None], c["u0"][None]

    def refused(call, match=None):
        with pytest.raises(kra.KoopmanHipError, match=match) as e:
            call()
        assert e.value.code == F.KP_ERR_ARG, e.value
    refused(lambda: dev.simulate(ref, np.zeros((0, 3)), np.zeros((0, 2))), "nb and nref")              # nb = 0
    refused(lambda: dev.simulate(ref[:0], y0, u0), "nb and nref")                                        # nref = 0
    refused(lambda: dev.simulate(np.zeros((25000, 1)), y0, u0), "bytes of LDS")                          # 200 KB of reference
    with pytest.raises(ValueError, match="y0_sc"):
        dev.simulate(ref, np.zeros((1, 2)), u0)
    with pytest.raises(ValueError, match="u0_sc"):
        dev.simulate(ref, y0, np.zeros((1, 3)))
    with pytest.raises(ValueError, match="ref_sc"):
        dev.simulate(np.zeros((NREF, 2)), y0, u0)
    with pytest.raises(ValueError, match="ref_sc"):
        dev.simulate(np.zeros((2, NREF, 1)), y0, u0)                                                     # two references, one trial
    U, Y, info, sd, st = dev.simulate(ref, y0, u0)                                                       # (the controller itself is fine)
    assert st[0] == F.KP_OK
