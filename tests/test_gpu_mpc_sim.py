"""GPU tests of kp_mpc_simulate (Mpc.simulate, Kmpc.run_simulations): whole closed loops with the identified model as
the plant, one workgroup per trial, one launch.

Acceptance check: teacher-forced parity.  Every recorded step k of a device run is replayed on its own recorded inputs:
the oracle's ko.mpc_step on (Z[k-1], U[k-1], reference window) gives U[k] to 1e-8 (the tolerance of test_gpu_mpc.py),
its pinned first row is the recorded U[k-1] to 1e-9, the numpy model step on (Z[k-1], U[k-1]) gives Y[k] to
1e-12 max(1, |Y|), and ko.econ_full(Y[k-1]) gives Z[k-1] to 1e-13.  A loop that carries a wrong state, window or input
from one step to the next fails one of the four at the step where it happens.

Free-running runs are compared with the host loop Kmpc.run_simulation.  Two correct closed loops drift apart by the
rounding of their QP solves fed back through the plant; that noise is MEASURED here between run_simulation and the
oracle's own loop (ko.mpc_step + the numpy model step) on the same 40 steps of the block-M, and the device loop has to
stay within 10 times it (scaled units, the larger of the Y and U differences).  Measured on an MI355X: noise 1.85e-11,
so the bound is 1.85e-10; the device loop differs from run_simulation by 7.7e-13 (U; Y 8.0e-14), the iters = 2 loop
from a host loop of step_zeta by 2.8e-12.  The `free_run` fixture measures the noise again on every run and prints it."""
import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from test_gpu_fit import make_basis
from test_gpu_mpc import arm_models, example_control_setup, make_mpc  # noqa: F401  (arm_models: a fixture)

pytestmark = pytest.mark.gpu


# ---- models ------------------------------------------------------------------------------------------------------
def model_step(mt, A, B, m, z, u):
    """z+ = A z + B u (linear) or A z + sum_i u_i B_i z (bilinear)."""
    return A @ z + (B @ u if mt == "linear" else ko.beta_bilinear(B, z, m) @ u)


# (n, poly degree, m, Np, model type, nproj): N = 4, 6, 10; nvar = 3 (odd), 14 (even), 36 (above 32)
SYNTH = [(1, 3, 1, 3, "linear", 1), (1, 3, 1, 3, "bilinear", 1), (2, 2, 2, 7, "linear", 1), (2, 2, 2, 7, "bilinear", 2),
         (3, 2, 3, 12, "linear", 2), (3, 2, 3, 12, "bilinear", 1)]


def synth_case(n, deg, m, Np, mt, nproj, seed=11):
    """A poly dictionary over n outputs with a random model: ||A||_2 = 0.8, B small, C = [I 0]; inputs in [-1, 1] with a
    slope limit, the last nproj outputs tracked."""
    dic = ko.build_dictionary(mt, n, m, ["poly"], [deg])
    N = dic.N
    rng = np.random.default_rng(seed + 100 * n + 10 * m + (mt == "bilinear"))
    A = rng.standard_normal((N, N))
    A *= 0.8 / np.linalg.norm(A, 2)
    B = 0.1 * rng.standard_normal((N, m if mt == "linear" else N * m))
    C = np.hstack([np.eye(n), np.zeros((n, N - n))])
    s = ko.MpcSetup(model_type=mt, A=A, B=B, m=m, Np=Np, projmtx=C[-nproj:], cost_running=1.0, cost_terminal=10.0,
                    cost_input=0.01, input_bounds=np.tile([-1.0, 1.0], (m, 1)), slope_lim=0.3, smooth_lim=None, n=n)
    return dic, s


def synth_inputs(s, nb, nref, seed=5):
    rng = np.random.default_rng(seed)
    ref = 0.3 * rng.standard_normal((nb, nref, s.projmtx.shape[0]))
    return ref, 0.4 * rng.uniform(-1, 1, (nb, s.n)), 0.5 * rng.uniform(-1, 1, (nb, s.m))


def check_teacher_forced(dic, s, ref_sc, U, Y, Z, steps, qp_every=1):
    """The four acceptance checks on the recorded steps 1 .. steps of one trial (the oracle's QP on every qp_every-th)."""
    n, Np = s.n, s.Np
    assert steps >= 1
    Zo = ko.econ_full(dic, Y[:steps])
    assert np.abs(Zo - Z[:steps]).max() < 1e-13
    for k in range(1, steps + 1):
        z, up = Z[k - 1], U[k - 1]
        z1 = model_step(s.model_type, s.A, s.B, s.m, z, up)
        assert np.abs(z1[:n] - Y[k]).max() <= 1e-12 * max(1.0, np.abs(Y[k]).max()), k
        if (k - 1) % qp_every == 0:
            Uo, _ = ko.mpc_step(s, z, up, ref_sc[k - 1:k + Np])
            assert np.abs(Uo[1] - U[k]).max() < 1e-8, k
            assert np.abs(Uo[0] - up).max() < 1e-9, k               # the pinned first input is the recorded previous one


@pytest.fixture(scope="module")
def arm_cases(ctx, arm, golden, arm_models):
    """The example_control.m controllers on the oracle's arm fits: (dic, setup, Mpc, Basis), the scaled block-M rows 0..40
    and the scaled start of the stored run."""
    ref = golden["blockM_ref"]["y"][:41]
    ysc = (ref - arm["scale"]["y_offset"][-2:]) / arm["scale"]["y_factor"][-2:]
    y0 = ko.scaledown(arm["scale"], "y", golden["arm_blockM"]["bilin_Y"][0])
    u0 = ko.scaledown(arm["scale"], "u", np.zeros(3))
    out = {"ref": ysc, "y0": y0, "u0": u0}
    for mt in ("bilinear", "linear"):
        dic, mdl = arm_models[mt]
        s = example_control_setup(arm, mt, dic, mdl)
        out[mt] = (dic, s, make_mpc(ctx, s), make_basis(ctx, dic))
    return out


# ---- teacher-forced parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", ["bilinear", "linear"])
def test_teacher_forced_parity_on_the_arm_controller(arm_cases, mt):
    dic, s, mpc, b = arm_cases[mt]
    assert mpc.N == 34 and mpc.m == 3 and mpc.Np == 10 and mpc.nvar == 30
    ref = arm_cases["ref"]
    U, Y, Z, sd, st = mpc.simulate(b, ref, arm_cases["y0"][None], arm_cases["u0"][None])
    assert st[0] == F.KP_OK and sd[0] == 40 and np.isfinite(U).all() and np.isfinite(Y).all() and np.isfinite(Z).all()
    assert (U[0, 0] == arm_cases["u0"]).all() and (Y[0, 0] == arm_cases["y0"]).all()
    check_teacher_forced(dic, s, ref, U[0], Y[0], Z[0], 40, qp_every=5)


@pytest.mark.parametrize("case", SYNTH, ids=lambda c: "n%d-deg%d-m%d-Np%d-%s-nproj%d" % c)
def test_teacher_forced_parity_on_small_models(ctx, case):
    dic, s = synth_case(*case)
    assert dic.N == {1: 4, 2: 6, 3: 10}[s.n] and s.m * s.Np in (3, 14, 36)
    mpc, b = make_mpc(ctx, s), make_basis(ctx, dic)
    nref = 9
    ref, y0, u0 = synth_inputs(s, 3, nref)
    U, Y, Z, sd, st = mpc.simulate(b, ref, y0, u0)
    assert (st == F.KP_OK).all() and (sd == nref - 1).all()
    for i in range(3):
        assert (U[i, 0] == u0[i]).all() and (Y[i, 0] == y0[i]).all()
        check_teacher_forced(dic, s, ref[i], U[i], Y[i], Z[i], nref - 1)


# ---- free-running against the existing routes ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kmpc_arm(ctx, golden):
    """example_control.m:15-40 through the host mirrors: Ksysid fit of the arm data, the bilinear controller."""
    g = golden["arm_data"]
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()
    kw = dict(horizon=10, input_bounds=[-7 * np.pi / 8, 7 * np.pi / 8], input_slopeConst=1e-1, input_smoothConst=None,
              cost_running=10, cost_terminal=100, cost_input=0.1 * np.array([3e-2, 2e-2, 1e-2]), projmtx=ks.model["C"][-2:, :])
    return ks, kra.Kmpc(ks, state_bounds=None, **kw), kw


@pytest.fixture(scope="module")
def free_run(kmpc_arm, golden):
    """40 steps of the block-M: the host loop run_simulation, the oracle's own loop on the same model, and the noise
    between the two in scaled units - the yardstick of the free-running comparisons (bound = 10 x noise)."""
    ks, mpc, _ = kmpc_arm
    ref = golden["blockM_ref"]["y"][:41]
    y0 = golden["arm_blockM"]["bilin_Y"][0]
    host = mpc.run_simulation(ref, y0, np.zeros(3))
    assert host["Y"].shape == (41, 6)
    sc = ks.params["scale"]
    dic = ko.Dictionary("bilinear", 6, 3, ko.make_basis(6, ["poly"], [3]), ks.basis["pcs"])
    s = ko.MpcSetup("bilinear", ks.model["A"], ks.model["B"], 3, 10, ks.model["C"][-2:, :], 10.0, 100.0,
                    0.1 * np.array([3e-2, 2e-2, 1e-2]),
                    np.stack([(np.full(3, -7 * np.pi / 8) - sc["u_offset"]) / sc["u_factor"],
                              (np.full(3, 7 * np.pi / 8) - sc["u_offset"]) / sc["u_factor"]], axis=1),
                    1e-1 * sc["u_factor"].mean(), None, None, 6)
    ysc = mpc.scaledown_ref(ref)
    Yo, Uo = [ks.scaledown_y(y0)], [ks.scaledown_u(np.zeros(3))]
    for k in range(1, 41):
        z = ko.econ_full(dic, Yo[-1][None, :])[0]
        Uk, _ = ko.mpc_step(s, z, Uo[-1], ysc[k - 1:k + 10])
        Yo.append(model_step("bilinear", s.A, s.B, 3, z, Uo[-1])[:6])
        Uo.append(Uk[1])
    noise = max(np.abs(ks.scaledown_y(host["Y"]) - np.array(Yo)).max(), np.abs(ks.scaledown_u(host["U"]) - np.array(Uo)).max())
    print("free-running noise (run_simulation vs the oracle's loop, 40 steps, scaled units): %.3e; bound %.3e" % (noise, 10 * noise))
    return {"ref": ref, "y0": y0, "host": host, "noise": noise, "bound": 10.0 * noise, "ysc": ysc}


def test_run_simulations_matches_run_simulation_free_running(kmpc_arm, free_run):
    ks, mpc, _ = kmpc_arm
    host = free_run["host"]
    res = mpc.run_simulations([free_run["ref"]], free_run["y0"][None], np.zeros((1, 3)))
    assert len(res) == 1
    dev = res[0]
    assert set(dev) == set(host) | {"steps_done"} and dev["steps_done"] == 40
    for k in ("T", "U", "Y", "K", "R", "Z", "comp_time"):
        assert dev[k].shape == host[k].shape, k
    assert (dev["K"] == host["K"]).all() and np.abs(dev["T"] - host["T"]).max() < 1e-12
    assert np.abs(dev["R"] - host["R"]).max() < 1e-12
    dY = np.abs(ks.scaledown_y(dev["Y"]) - ks.scaledown_y(host["Y"])).max()
    dU = np.abs(ks.scaledown_u(dev["U"]) - ks.scaledown_u(host["U"])).max()
    print("device loop vs run_simulation: dY %.3e dU %.3e (bound %.3e)" % (dY, dU, free_run["bound"]))
    assert max(dY, dU) <= free_run["bound"]
    assert (dev["comp_time"] > 0).all() and np.ptp(dev["comp_time"]) == 0
    # a reference given as {t, y} goes through resample_ref; one given for every trial serves all of them
    t = np.arange(41) * ks.params["Ts"]
    two = mpc.run_simulations({"t": t, "y": free_run["ref"]}, np.stack([free_run["y0"]] * 2), None)
    assert len(two) == 2
    for r in two:
        assert np.abs(ks.scaledown_y(r["Y"]) - ks.scaledown_y(dev["Y"])).max() <= free_run["bound"]


def test_iterated_linearisation_matches_a_host_loop_of_step_zeta(kmpc_arm, free_run):
    ks, mpc, _ = kmpc_arm
    ysc = free_run["ysc"]
    y0, u0 = ks.scaledown_y(free_run["y0"]), ks.scaledown_u(np.zeros(3))
    U, Y, Z, sd, st = mpc.dev.simulate(ks.basis_dev, ysc, y0[None], u0[None], iters=2)
    assert st[0] == F.KP_OK and sd[0] == 40
    A, B = ks.model["A"], ks.model["B"]
    Yh, Uh = [y0], [u0]
    for k in range(1, 41):
        Us, z, s_ = mpc.dev.step_zeta(ks.basis_dev, Yh[-1], Uh[-1], mpc._pad_ref(ysc[k - 1:k + 10]), 2)
        assert s_ == 0
        Yh.append(model_step("bilinear", A, B, 3, z, Uh[-1])[:6])
        Uh.append(Us[1])
    d = max(np.abs(Y[0] - np.array(Yh)).max(), np.abs(U[0] - np.array(Uh)).max())
    print("iters = 2, device loop vs host loop of step_zeta: %.3e (bound %.3e)" % (d, free_run["bound"]))
    assert d <= free_run["bound"]


# ---- batch independence ---------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_a_trial_does_not_depend_on_the_batch_it_runs_in(arm_cases):
    dic, s, mpc, b = arm_cases["bilinear"]
    rng = np.random.default_rng(3)
    nb, nref = 5, 14
    ref = np.stack([arm_cases["ref"][i:i + nref] for i in (0, 3, 9, 20, 27)])
    y0 = arm_cases["y0"] + 0.05 * rng.standard_normal((nb, 6))
    u0 = arm_cases["u0"] + 0.1 * rng.standard_normal((nb, 3))
    U, Y, Z, sd, st = mpc.simulate(b, ref, y0, u0)
    assert (st == F.KP_OK).all() and (sd == nref - 1).all()
    for i in range(nb):
        U1, Y1, Z1, sd1, st1 = mpc.simulate(b, ref[i:i + 1], y0[i:i + 1], u0[i:i + 1])
        assert same_bits(U1[0], U[i]) and same_bits(Y1[0], Y[i]) and same_bits(Z1[0], Z[i]) and sd1[0] == sd[i], i
    # one reference for all trials = the same reference repeated per trial
    Us, Ys, Zs, sds, sts = mpc.simulate(b, ref[1], y0, u0)
    Ur, Yr, Zr, sdr, str_ = mpc.simulate(b, np.stack([ref[1]] * nb), y0, u0)
    assert same_bits(Us, Ur) and same_bits(Ys, Yr) and same_bits(Zs, Zr) and (sds == sdr).all() and (sts == str_).all()
    assert not same_bits(Us[0], Us[1])


def test_more_trials_than_are_resident(ctx):
    dic, s = synth_case(2, 2, 2, 7, "bilinear", 2)
    assert dic.N == 6
    mpc, b = make_mpc(ctx, s), make_basis(ctx, dic)
    nref, nb = 6, 1100
    ref, y0, u0 = synth_inputs(s, 11, nref, seed=9)
    idx = np.arange(nb) % 11
    U, Y, Z, sd, st = mpc.simulate(b, ref[0], y0[idx], u0[idx])
    assert (st == F.KP_OK).all() and (sd == nref - 1).all()
    for j in range(11):
        U1, Y1, Z1, _, _ = mpc.simulate(b, ref[0], y0[j:j + 1], u0[j:j + 1])
        rows = np.nonzero(idx == j)[0]
        assert len(rows) == 100
        assert all(same_bits(U[i], U1[0]) and same_bits(Y[i], Y1[0]) and same_bits(Z[i], Z1[0]) for i in rows), j
    assert not same_bits(Y[0], Y[1])


SIM_PINNED_BYTES = 4 << 20      # up to here a call's results come back in one copy through page-locked scratch


def sim_block_bytes(nb, nref, nproj, ny, m, aux_w, shared):
    """The device block of one kp_mpc_simulate / kp_nmpc_simulate call (kp_sim_loop.h):
    [ref | y0 | u0] | U | Y | aux | steps_done, status - doubles, the 2 nb ints rounded up to whole doubles."""
    n_in = (1 if shared else nb) * nref * nproj + nb * ny + nb * m
    n_out = nb * nref * m + nb * nref * ny + nb * (nref - 1) * aux_w + (2 * nb + 1) // 2
    return 8 * (n_in + n_out)


def copies_of(big, one, rows):
    """Every row of `big` listed in `rows` has the bits of one[0]."""
    return big[rows].tobytes() == np.broadcast_to(one[:1], big[rows].shape).tobytes()


def test_results_copied_straight_to_the_callers_arrays(ctx):
    """A call above SIM_PINNED_BYTES copies each output straight into the caller's array; every trial of it has the bits of
    the same start run alone, which comes back through the page-locked scratch."""
    dic, s = synth_case(2, 2, 2, 7, "bilinear", 2)
    mpc, b = make_mpc(ctx, s), make_basis(ctx, dic)
    nref, nd = 6, 10
    size = lambda nb: sim_block_bytes(nb, nref, 2, 2, 2, dic.N, True)
    nb = nd * (SIM_PINNED_BYTES // (size(nd) - size(0)) + 1)
    assert size(nb) > SIM_PINNED_BYTES >= size(nb - 2 * nd) and size(1) <= SIM_PINNED_BYTES, (nb, size(nb))
    ref, y0, u0 = synth_inputs(s, nd, nref, seed=9)
    idx = np.arange(nb) % nd
    U, Y, Z, sd, st = mpc.simulate(b, ref[0], y0[idx], u0[idx])
    assert (st == F.KP_OK).all() and (sd == nref - 1).all()
    for j in range(nd):
        U1, Y1, Z1, sd1, st1 = mpc.simulate(b, ref[0], y0[j:j + 1], u0[j:j + 1])
        rows = np.nonzero(idx == j)[0]
        assert len(rows) == nb // nd
        assert copies_of(U, U1, rows) and copies_of(Y, Y1, rows) and copies_of(Z, Z1, rows), j
        assert copies_of(sd, sd1, rows) and copies_of(st, st1, rows), j
    assert not same_bits(Y[0], Y[1])


# ---- edges -------------------------------------------------------------------------------------------------------------
def test_short_references(arm_cases):
    dic, s, mpc, b = arm_cases["bilinear"]
    ref, y0, u0 = arm_cases["ref"], arm_cases["y0"][None], arm_cases["u0"][None]
    U, Y, Z, sd, st = mpc.simulate(b, ref[:1], y0, u0)                    # nref = 1: no step
    assert U.shape == (1, 1, 3) and Y.shape == (1, 1, 6) and Z.shape == (1, 0, 34) and sd[0] == 0 and st[0] == F.KP_OK
    assert (U[0, 0] == u0[0]).all() and (Y[0, 0] == y0[0]).all()
    for nref in (2, 3):                                                   # one step, two steps: windows padded as _pad_ref does
        U, Y, Z, sd, st = mpc.simulate(b, ref[:nref], y0, u0)
        assert sd[0] == nref - 1 and st[0] == F.KP_OK
        check_teacher_forced(dic, s, ref[:nref], U[0], Y[0], Z[0], nref - 1)
        Us, z, s_ = mpc.step_zeta(b, y0[0], u0[0], ko.pad_ref(ref[:nref], s.Np))
        assert s_ == 0 and np.abs(Us[1] - U[0, 1]).max() < 1e-9 and np.abs(z - Z[0, 0]).max() < 1e-13
    U, Y, Z, sd, st = mpc.simulate(b, ref[:4], y0, u0, want_Z=False)
    assert Z is None and sd[0] == 3


# ---- failure stays local -------------------------------------------------------------------------------------------------
def test_a_failed_qp_ends_its_own_trial_only(arm_cases):
    dic, s, mpc, b = arm_cases["bilinear"]
    nref = 8
    ref = arm_cases["ref"][:nref]
    y0 = np.stack([arm_cases["y0"]] * 3)
    u0 = np.stack([arm_cases["u0"], np.array([5.0, 0.0, 0.0]), arm_cases["u0"] + 0.05])   # the middle one: outside the input box
    U, Y, Z, sd, st = mpc.simulate(b, ref, y0, u0)
    assert st[1] == F.KP_ERR_QP_FAIL and sd[1] == 0
    assert (U[1, 0] == u0[1]).all() and (Y[1, 0] == y0[1]).all()
    assert np.isnan(U[1, 1:]).all() and np.isnan(Y[1, 1:]).all() and np.isnan(Z[1]).all()
    for i in (0, 2):
        U1, Y1, Z1, sd1, st1 = mpc.simulate(b, ref, y0[i:i + 1], u0[i:i + 1])
        assert st[i] == F.KP_OK and sd[i] == nref - 1 and st1[0] == F.KP_OK
        assert same_bits(U1[0], U[i]) and same_bits(Y1[0], Y[i]) and same_bits(Z1[0], Z[i]), i


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(ctx, arm, arm_models, arm_cases):
    dic, s, _, b = arm_cases["bilinear"]
    ref, y0, u0 = arm_cases["ref"][:5], arm_cases["y0"][None], arm_cases["u0"][None]
    mpc = make_mpc(ctx, s)                                              # (its own controller: the bounds stay on it)

    def refused(call):
        with pytest.raises(kra.KoopmanHipError) as e:
            call()
        assert e.value.code == F.KP_ERR_ARG, e.value
    refused(lambda: mpc.simulate(b, ref, np.zeros((0, 6)), np.zeros((0, 3))))                       # nb = 0
    dic_d = ko.build_dictionary("bilinear", 15, 3, ["poly"], [2])                                   # zeta of a model with one delay
    refused(lambda: mpc.simulate(make_basis(ctx, dic_d), ref, y0, u0))
    dic_s, s_s = synth_case(3, 2, 3, 12, "bilinear", 1)                                             # N = 10, not 34
    refused(lambda: mpc.simulate(make_basis(ctx, dic_s), ref, np.zeros((1, 3)), u0))
    U, Y, Z, sd, st = mpc.simulate(b, ref, y0, u0)                                                  # (the controller itself is fine)
    assert st[0] == F.KP_OK
    mpc.set_state_bounds(np.full(6, -10.0), np.full(6, 10.0))
    refused(lambda: mpc.simulate(b, ref, y0, u0))


def test_run_simulations_with_state_bounds_takes_the_host_loop(kmpc_arm, free_run):
    ks, _, kw = kmpc_arm
    mpc = kra.Kmpc(ks, state_bounds=[-100.0, 100.0], **kw)
    ref, y0 = free_run["ref"][:6], free_run["y0"]
    host = mpc.run_simulation(ref, y0, np.zeros(3))
    res = mpc.run_simulations([ref], y0[None], None)
    assert len(res) == 1 and set(res[0]) == set(host) | {"steps_done"} and res[0]["steps_done"] == 5
    for k in ("T", "U", "Y", "K", "R", "Z"):
        assert res[0][k].shape == host[k].shape and np.abs(res[0][k] - host[k]).max() < 1e-9, k
