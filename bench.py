#!/usr/bin/env python3
"""bench.py — headline benchmark of the Koopman hot path on MI355X.

Metric (BASELINE.json): EDMD snapshot-pairs/s (+ MPC steps/s reported beside it) for the
3-link-arm bilinear model.  Workload at N=1 = BASELINE configs[1]: bilinear Koopman fit,
poly degree 3 (N=84, W=336), 1e5 synthetic snapshot pairs, one MI355X.  A "step" is one
complete fit (fused lift+Gram kernel, partial reduction, Cholesky solve -> K) of the
resident snapshot matrix.  Inputs are uploaded to HBM before the timed region.

Multi-GPU (N>1): one process per GPU (launched by torch.distributed.run, or spawned here when bench.py is
started directly with --gpus N), torch-free: the RCCL communicator lives behind the C ABI (kp_comm_*).  Every rank
fits its own snapshot matrix of the same shape (the units of the reference's sweeps are independent fits: lasso grid
Ksysid.m:1372-1387, evaluate_rand_models.m:45-144) => weak scaling, no data-path collective; one RCCL all-gather of
the resulting K matrices closes the timed region.  The sharded sections (64-value lasso grid, 1024 random systems)
report their own whole-job numbers per N.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F64_MFMA_TFLOPS = 78.6   # MI355X FP64 matrix (vendor datasheet; the guide lists no f64 row)
PEAK_HBM_GBS = 8000.0


COMPACT_LINE_LIMIT = 4000     # bytes; the driver parses the LAST stdout line and lost round 5's 21.7 KB one


def _r(x, sig=6):
    """Numbers of the compact line: `sig` significant digits."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return float(f"{x:.{sig}g}")
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def compact_line(res):
    """The ONE stdout line: the contract's keys, `roofline`, `cpu_baseline` and a few-number summary of each secondary
    section, well under COMPACT_LINE_LIMIT bytes.  Everything else (`res` whole) goes to stderr and to bench_detail.json
    (emit_result).  Pure function of `res` so that tests/test_bench_line.py can size it without a GPU."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data")
    out = {k: res.get(k) for k in keep}
    cfg = res.get("config", {})
    out["config"] = {k: cfg[k] for k in ("workload", "snapshots_per_gpu", "W", "parallelism", "comm") if k in cfg}
    rf = res.get("roofline")
    if rf:
        out["roofline"] = {k: rf[k] for k in ("kernel", "bound", "ms", "achieved", "peak", "unit", "frac", "traffic",
                                              "executed_flop_per_launch", "dense_equivalent_flop_per_launch", "dense_equivalent_frac",
                                              "algorithmic_bytes_per_launch") if k in rf}
    cb = res.get("cpu_baseline")
    if cb:
        o = {k: cb[k] for k in ("value", "unit", "cores", "kind") if k in cb}
        o["sample"] = str(cb.get("sample", ""))[:200]
        if "one_thread" in cb:
            o["one_thread_value"] = cb["one_thread"].get("value")
        if "mpc" in cb:
            o["mpc_steps_per_s"] = cb["mpc"].get("value")
        out["cpu_baseline"] = o
    for k in ("fit_latency_ms", "fit_with_K_fetched_ms"):
        if k in res:
            out[k] = res[k]
    if "kernel_ms" in res:
        out["kernel_ms"] = {k: res["kernel_ms"].get(k) for k in ("gram", "gram_reduce", "solve")}
    m = res.get("mpc")
    if m:
        out["mpc"] = {k: m[k] for k in ("single_steps_per_s", "single_kernel_us", "closed_loop_steps_per_s", "closed_loop_us_per_step",
                                        "closed_loop_kernel_us", "batch_problems_per_s") if k in m}
    a = res.get("mpc_arm_blockM")
    if a:
        out["mpc_arm"] = {k: a[k] for k in ("steps_per_s", "controller_us_per_step", "get_koopman_end_to_end_ms") if k in a}
    pts = {}
    for sec in ("width_points", "snapshot_count_points", "wide_dictionaries"):
        for name, w in (res.get(sec) or {}).items():
            if isinstance(w, dict) and "error" not in w:
                r_ = w.get("roofline", {})
                pts[name] = [w.get("gram_ms"), r_.get("frac"), w.get("ms_per_fit")]
    if pts:
        out["points"] = dict(pts, _fields="[gram_ms, executed frac of f64 MFMA peak, ms_per_fit]")
    l = res.get("lasso_grid")
    if l:
        out["lasso_grid"] = {k: l[k] for k in ("values", "values_per_s", "seconds", "n_gpus") if k in l}
    sw = res.get("rand_sweep")
    if sw:
        out["rand_sweep"] = {k: sw[k] for k in ("systems", "systems_per_s", "seconds", "n_gpus") if k in sw}
    sh = res.get("snapshot_sharded_fit")
    if sh:
        out["snapshot_sharded_fit"] = {k: (v.get("pairs_per_s") if isinstance(v, dict) else v) for k, v in sh.items()}
    oc = res.get("one_caller")
    if oc:
        out["one_caller"] = ({"error": str(oc["error"])[:120]} if "error" in oc else
                             {"n_devices": len(oc.get("device_ids", [])),
                              "lasso_values_per_s": (oc.get("lasso_grid") or {}).get("values_per_s"),
                              "rand_systems_per_s": (oc.get("rand_sweep") or {}).get("systems_per_s")})
    out["detail"] = "bench_detail.json (also one line on stderr)"
    out = _r(out)
    line = json.dumps(out, separators=(",", ":"))
    if len(line) > COMPACT_LINE_LIMIT:              # never again a line the driver cannot take: shed the summaries first
        for k in ("points", "one_caller", "snapshot_sharded_fit", "mpc_arm", "rand_sweep", "lasso_grid", "mpc", "kernel_ms"):
            out.pop(k, None)
            line = json.dumps(out, separators=(",", ":"))
            if len(line) <= COMPACT_LINE_LIMIT:
                break
    return line


def emit_result(res, compact=True):
    """Detail -> stderr (one line) and bench_detail.json / gpurun_out/bench_detail.json; the compact line -> stdout, last."""
    full = json.dumps(res)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        try:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "bench_detail.json"), "w") as f:
                f.write(full + "\n")
        except OSError:
            pass
    print(full, file=sys.stderr, flush=True)
    print(compact_line(res) if compact else full, flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: each 2-D array as d/<name>.npy in float64.  The total stays within `limit`: an array over its share
    keeps a fixed seeded sample of its columns (the same columns for the same shape, so two builds compare entry for entry)."""
    os.makedirs(d, exist_ok=True)
    share = limit // len(arrays)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        if a.nbytes > share:
            keep = share // (a.shape[0] * 8)
            a = a[:, np.sort(np.random.default_rng(0).choice(a.shape[1], size=keep, replace=False))]
        np.save(os.path.join(d, name + ".npy"), a)


def synth_pairs(Ns, nz=6, m=3, seed=0):
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(-1, 1, (Ns, nz)); u = rng.uniform(-1, 1, (Ns, m))
    Mx = rng.standard_normal((nz + m, nz)) * 0.3
    beta = np.clip(alpha + 0.05 * np.tanh(np.hstack([alpha, u]) @ Mx), -1, 1)
    return alpha, beta, u


def cpu_baseline(Ns_sample, degree, seconds=8.0):
    """The oracle's restatement of get_Koopman on the host cores, on a bounded sample of the same workload: the lift of
    every row (Ksysid.m:1030-1065) + `Px \\ Py` (:1069; MATLAB's mldivide on a rectangular system is a Householder QR
    solve).  The CPU backend of the same C ABI (oracle/koopman_cpu_abi.c over oracle/koopman_oracle_c.c, OpenMP), called exactly
    as the GPU library is (kp_create -> kp_basis_create -> kp_snapshots_upload -> kp_fit), else numpy + LAPACK gelsy.  Two
    rows: all host cores (`value`) and one thread (the reference's interpreter is single threaded apart from BLAS)."""
    alpha, beta, u = synth_pairs(Ns_sample, seed=123)
    try:
        from oracle import cpu_abi, koopman_oracle as ko
        cl = cpu_abi.lib()
        exps = ko.poly_exponents(6, degree)[6:]
        fitobj = cpu_abi.CpuFit("bilinear", 6, 3, exps, alpha, beta, u)     # kp_create / kp_basis_create / kp_snapshots_upload
        W = fitobj.W

        def timed(limit):
            t0 = time.perf_counter(); reps = 0
            while True:
                fitobj.fit(); reps += 1                                     # kp_fit: lift of every row + Householder QR
                if time.perf_counter() - t0 > limit:
                    break
            return (time.perf_counter() - t0) / reps, reps
        # "all cores" = the cores this process may run on (a 256-thread OpenMP team on a box that grants fewer turns the
        # per-column barriers of the QR into time slicing), at most 32
        try:
            avail = len(os.sched_getaffinity(0))
        except AttributeError:
            avail = os.cpu_count() or 1
        all_cores = max(1, min(cl.ko_max_threads(), avail, 32))
        cl.ko_set_threads(all_cores)
        dt_all, reps_all = timed(seconds)
        cl.ko_set_threads(1)
        dt_1, reps_1 = timed(seconds)
        cl.ko_set_threads(all_cores)
        fitobj.close()
        how = "CPU backend of the same C ABI (oracle/libkoopman_cpu.so: kp_fit = per-row lift + Householder QR, OpenMP)"
    except (ImportError, OSError):
        import scipy.linalg as sla
        import threadpoolctl
        from oracle import koopman_oracle as ko
        pairs = {"alpha": alpha, "beta": beta, "u": u}
        dic = ko.build_dictionary("bilinear", 6, 3, ["poly"], [degree])
        W = dic.W

        def one():
            Px, Py = ko.px_py(dic, pairs)
            return sla.lstsq(Px, Py, lapack_driver="gelsy", check_finite=False)[0]

        def timed(limit):
            t0 = time.perf_counter(); reps = 0
            while True:
                one(); reps += 1
                if time.perf_counter() - t0 > limit:
                    break
            return (time.perf_counter() - t0) / reps, reps
        all_cores = max([p_.get("num_threads", 1) for p_ in threadpoolctl.threadpool_info()] + [1])
        dt_all, reps_all = timed(seconds)
        with threadpoolctl.threadpool_limits(1):
            dt_1, reps_1 = timed(seconds)
        how = "numpy lift + LAPACK QR (gelsy)"
    return {"value": Ns_sample / dt_all, "unit": "snapshot-pairs/s", "cores": int(all_cores), "kind": "port",
            "sample": f"{reps_all} x get_Koopman, {how}, on {Ns_sample} pairs, W={W}, {dt_all*1e3:.0f} ms each",
            "one_thread": {"value": Ns_sample / dt_1, "cores": 1,
                           "sample": f"{reps_1} x the same on one thread, {dt_1*1e3:.0f} ms each"}}


def mpc_problem(kra, ctx, basis, snaps, horizon=10):
    """Bilinear Kmpc on the model of the synthetic fit (N=84), example_control.m:20-28 settings."""
    from koopman_realizations_amd.device import Mpc
    N, m = basis.N, 3
    K = kra.fit(ctx, basis, snaps)[0]
    A = np.asfortranarray(K[:N, :N].T); B = np.asfortranarray(K[N:, :N].T)      # Ksysid.m:1258-1259
    proj = np.zeros((2, N)); proj[0, 4] = proj[1, 5] = 1.0                      # C(end-1:end,:)
    u_fac = 2.8
    setup = dict(A=A, B=B, N=N, m=m, Np=horizon, proj=proj, q_run=10.0, q_term=100.0,
                 r=0.1 * np.array([3e-2, 2e-2, 1e-2]), lo=np.full(3, -7 * np.pi / 8 / u_fac), hi=np.full(3, 7 * np.pi / 8 / u_fac),
                 slope=1e-1 * u_fac)
    mpc = Mpc(ctx, "bilinear", A, B, horizon, proj, setup["q_run"], setup["q_term"], setup["r"], setup["lo"], setup["hi"], setup["slope"])
    return mpc, setup


def mpc_inputs(nb, seed=7):
    rng = np.random.default_rng(seed)
    zeta = rng.uniform(-0.6, 0.6, (nb, 6))
    u_prev = rng.uniform(-0.3, 0.3, (nb, 3))
    th = rng.uniform(0, 2 * np.pi, (nb, 1)) + 0.15 * np.arange(11)[None, :]
    ref = np.stack([zeta[:, [4]] + 0.2 * (np.cos(th) - np.cos(th[:, :1])), zeta[:, [5]] + 0.2 * (np.sin(th) - np.sin(th[:, :1]))], axis=2)
    return zeta, u_prev, ref.reshape(nb, -1)      # Yr = vec(ref') per problem


def bench_mpc(ctx, kra, basis, snaps, args):
    """MPC steps/s: (a) latency-bound stream of single steps on INDEPENDENT random states (lift + assembly + QP in
    one launch, host round trip per step, as Ksim.run_trial_mpc calls it), (b) batched independent problems,
    (c) a 300-step closed loop (the host plant update is inside the timed loop)."""
    from koopman_realizations_amd import _ffi as F
    mpc, setup = mpc_problem(kra, ctx, basis, snaps)
    zeta, u_prev, Yr = mpc_inputs(max(args.mpc_steps, args.mpc_batch))
    for i in range(5):
        mpc.step_zeta(basis, zeta[i], u_prev[i], Yr[i])
    t0 = time.perf_counter(); ok = 0; kern = []
    for i in range(args.mpc_steps):
        U, z, st = mpc.step_zeta(basis, zeta[i], u_prev[i], Yr[i])
        ok += st == 0; kern.append(ctx.timer(2))
    dt1 = time.perf_counter() - t0
    # (c) the closed loop of BASELINE configs[2]: 300 steps, the identified model as the plant (Kmpc.run_simulation,
    # Kmpc.m:403-512), circular end-effector reference; consecutive QPs share most of their active set, which the
    # single-problem path uses as a warm start
    A_, B_, N_ = setup["A"], setup["B"], setup["N"]
    th = 0.05 * np.arange(args.mpc_steps + 12)
    cref = np.stack([0.3 * np.cos(th), 0.3 * np.sin(th)], axis=1)
    zc = np.zeros(6); zc[4] = 0.3
    uc = np.zeros(3)
    t0 = time.perf_counter(); okc = 0; kernc = []
    for k in range(args.mpc_steps):
        U, z, st = mpc.step_zeta(basis, zc, uc, cref[k:k + 11].reshape(-1))
        okc += st == 0; kernc.append(ctx.timer(2))
        if st != 0:
            break
        z1 = A_ @ z + sum(B_[:, i * N_:(i + 1) * N_] @ z * U[0, i] for i in range(3))
        zc = z1[:6]; uc = U[0]
    dtc = time.perf_counter() - t0
    # lifted states in the ABI's layout (one problem's N values contiguous = an N x nb column-major matrix, what a MATLAB caller
    # holds); kp_lift returns nb x N column-major, and re-laying 2.7 MB out inside every timed call cost 1.4 of its 3.0 ms
    Z = np.ascontiguousarray(basis.lift(F.LIFT_ECON, zeta[:args.mpc_batch]))
    mpc.step_batch(Z, u_prev[:args.mpc_batch], Yr[:args.mpc_batch])
    dtb = 1e30
    for _ in range(3):       # best of 3: one call is a few ms, so a single wall-clock sample is noisy
        t0 = time.perf_counter()
        Ub, stb = mpc.step_batch(Z, u_prev[:args.mpc_batch], Yr[:args.mpc_batch])
        dtb = min(dtb, time.perf_counter() - t0)
    return {"single_steps_per_s": args.mpc_steps / dt1, "single_us_per_step": dt1 / args.mpc_steps * 1e6,
            "single_kernel_us": float(np.mean(kern)) * 1e3, "single_solved": int(ok), "single_steps": args.mpc_steps,
            "closed_loop_steps_per_s": okc / dtc, "closed_loop_us_per_step": dtc / max(okc, 1) * 1e6,
            "closed_loop_kernel_us": float(np.mean(kernc)) * 1e3, "closed_loop_solved": int(okc),
            "batch_problems_per_s": args.mpc_batch / dtb, "batch": args.mpc_batch, "batch_kernel_ms": ctx.timer(2),
            "batch_problems_per_s_kernel_only": args.mpc_batch / (ctx.timer(2) * 1e-3),
            "batch_solved": int((stb == 0).sum()),
            "workload": "bilinear Kmpc, N=84 model of the synthetic fit, horizon 10, 30 variables x 126 rows (BASELINE configs[2] shape)",
            "reference_recorded": "MATLAB R2019a stored comp_time: median 8.7 ms/step (~104 steps/s), N=34, unknown PC",
            "_setup": (setup, basis.N, zeta[:20], u_prev[:20], Yr[:20])}


def bench_lasso(ctx, comm, kra, basis, snaps, n_values=64):
    """BASELINE configs[3]: the 64-value lasso grid on the bilinear fit (t/N log-spaced in [1e-2, 1e2];
    lasso = t/N, Ksysid.m:996), values dealt round-robin to the ranks, each rank handing its whole shard to ONE kp_fit
    call (snapshots lifted once, the shard's values batched on the device), final gather of the K stack over RCCL.
    Every rank fits the same snapshot matrix (as train_models does for every value)."""
    from koopman_realizations_amd import sweep, comm as kc
    W = basis.W
    vals = list(np.geomspace(1e-2, 1e2, n_values))
    fit_dev = lambda ls: kra.fit(ctx, basis, snaps, ls, fetch=False)      # the shard's K stack stays in HBM
    mine = sweep.shard_units(n_values, comm.rank, comm.world)
    per = (n_values + comm.world - 1) // comm.world
    kra.fit(ctx, basis, snaps, [vals[i] for i in mine[:1]], fetch=False)  # warm-up (allocations, RCCL channels)
    sweep.lasso_sweep_device(ctx, fit_dev, vals, W, comm, root=0)         # ... and every buffer at its final size
    comm.barrier()
    t0 = time.perf_counter()
    t_g = [0.0]
    _gather = kc.all_gather_fits

    def timed_gather(*a, **k):
        t1 = time.perf_counter(); r = _gather(*a, **k); t_g[0] = time.perf_counter() - t1
        return r
    kc.all_gather_fits = timed_gather
    try:
        # the stack goes to rank 0 ONLY (kp_comm_gather_fits: the other ranks send their share and return) - one host wants
        # the candidates of train_models, as in the reference (Ksysid.m:1370-1387)
        Ks = sweep.lasso_sweep_device(ctx, fit_dev, vals, W, comm, root=0)
    finally:
        kc.all_gather_fits = _gather
    comm.barrier()
    dt = kc.max_over_ranks(comm, time.perf_counter() - t0)
    per_rank = kc.all_gather_array(comm, np.array([ctx.timer(3), t_g[0] * 1e3]))       # device ms (lasso batch), gather ms of every rank
    if Ks is None:
        return None
    l1 = np.array([np.abs(K).sum() for K in Ks])
    t = np.array(vals) * basis.N
    active = int((l1 < l1.max() * (1 - 1e-9)).sum())
    return {"values": n_values, "seconds": dt, "values_per_s": n_values / dt, "ms_per_value": dt / n_values * 1e3, "W": W,
            "n_gpus": comm.world, "active_constraints": active,
            "budget_met": bool(np.all(l1 <= t * (1 + 1e-9) + 1e-12)),
            "device_ms_rank0": ctx.timer(3), "gather_ms_rank0": t_g[0] * 1e3, "_gemm": (ctx.timer(8), ctx.timer(9)) if ctx.timer(9) > 0 else None,
            "device_ms_per_rank": per_rank[:, 0].tolist(), "gather_ms_per_rank": per_rank[:, 1].tolist(),
            "gather": f"K stacks of the shards sent to rank 0 only ({comm.kind}; kp_comm_gather_fits), one DMA of {n_values * W * W * 8 / 1e6:.0f} MB into a page-locked block there",
            "workload": "64 lasso values (t/N log-spaced 1e-2..1e2) on the bilinear poly-3 fit, 1e5 pairs, sharded round-robin, "
                        "K stack gathered (BASELINE configs[3])"}


def bench_lasso_ill_conditioned(ctx, kra):
    """The lasso on a Gram matrix like those of the reference's own arm data (monomial dictionary on strongly correlated
    states: cond(G) ~ 1e10, as the arm data's): bilinear poly-2 dictionary on 6 states that are noisy mixtures of two latent signals, m = 3
    (W = 112), 12 000 pairs, budgets 0.5 and 0.1 |K_LS|_1 (solve_KoopmanQP, Ksysid.m:1095-1176).  The projected-gradient
    iteration cannot finish these (rounds 1-3: KP_ERR_NOT_CONVERGED after 0.6 s); kp_fit hands them to the regularisation-path
    homotopy (csrc/kp_lasso_path.hip).  Reported: wall time of the kp_fit call, the homotopy's share, budget met."""
    rng = np.random.default_rng(11)
    Ns = 12000
    ts = np.linspace(0.0, 60.0, Ns + 1)
    lat = np.stack([np.sin(0.9 * ts), np.cos(0.37 * ts + 0.4)], 1)
    Y = 0.8 * lat @ rng.uniform(-1, 1, (2, 6)) + 5e-3 * rng.standard_normal((Ns + 1, 6))
    u = rng.uniform(-1, 1, (Ns, 3))
    exps = kra.poly_exponent_table(6, 2)[6:]
    b = kra.Basis(ctx, "bilinear", 6, 3, [("poly", exps)])
    s_ = kra.Snapshots(ctx, np.ascontiguousarray(Y[:-1]), np.ascontiguousarray(Y[1:]), u)
    G, C = kra.fit_gram(ctx, b, s_)
    ev = np.linalg.eigvalsh((G + G.T) / 2)
    Kls = kra.fit(ctx, b, s_)[0]
    l1 = float(np.abs(Kls).sum())
    las = [0.5 * l1 / b.N, 0.1 * l1 / b.N]
    kra.fit(ctx, b, s_, las)                                                  # warm-up (allocations)
    t0 = time.perf_counter()
    Ks = kra.fit(ctx, b, s_, las)
    dt = time.perf_counter() - t0
    res = {"W": b.W, "pairs": Ns, "cond_G": float(ev[-1] / (ev[0] if ev[0] > 0 else 1e-6)), "budgets": "0.5 and 0.1 |K_LS|_1",
           "ms": dt * 1e3, "homotopy_ms": ctx.timer(11),
           "budget_met": bool(all(abs(np.abs(K).sum() - lv * b.N) <= 1e-9 * lv * b.N for K, lv in zip(Ks, las))),
           "nnz": [int((K != 0).sum()) for K in Ks],
           "workload": "synthetic arm-like data: 6 states = mixtures of 2 latent signals + 5e-3 noise, bilinear poly-2 dictionary"}
    s_.close(); b.close()
    return res


RAND_CHUNK = 128


def _rand_chunk(c):
    """Systems [128 c, 128 c + 128) of the generated sweep population (host, numpy; seeded per chunk so that every
    N-GPU run sees the same 1024 systems): Rsys(128 systems, 3 terms, degree_x 3, degree_u 2), 10 + 1 trials of 1001
    samples at Ts = 0.01 (Rsys.m:96-125, 136-150; the shipped data set's shape)."""
    from koopman_realizations_amd.rsys import Rsys
    r = Rsys(RAND_CHUNK, 3, 3, 2, seed=1000 + c)
    return Rsys.save_data(r.simulate_systems_fast(10.0, 0.01, 11, np.zeros((1, 1))))


def gen_rand_systems(chunks):
    """Generates the chunks in worker processes (fork, BEFORE this process touches the GPU)."""
    import multiprocessing as mp
    if not chunks:
        return {}
    nproc = min(len(chunks), max(1, min(len(os.sched_getaffinity(0)), os.cpu_count() or 2) - 1))
    if nproc == 1:
        return {c: _rand_chunk(c) for c in chunks}
    with mp.get_context("fork").Pool(nproc) as pool:
        return dict(zip(chunks, pool.map(_rand_chunk, chunks)))


def bench_rand_sweep(ctx, comm, kra, chunks, n_systems):
    """BASELINE configs[4]: evaluate_rand_models.m (linear deg 1..13, bilinear 1..6, nonlinear 1..4 fits + validation
    rollouts per random system) on n_systems DISTINCT generated systems, chunks of 128 dealt round-robin to the ranks,
    each rank's shard through the batched device path, final gather of the error tables."""
    from koopman_realizations_amd import sweep, comm as kc
    mine = [s_ for c in sorted(chunks) for s_ in chunks[c]]
    ids = [c * RAND_CHUNK + k for c in sorted(chunks) for k in range(RAND_CHUNK)]
    sweep.rand_models_sweep_batched(mine[:4], ctx)                           # warm-up
    if mine:
        sweep._stack_raw(mine, ctx)          # the context's page-locked gather buffers at their final size (untimed, like every
                                             # other buffer of the pipeline); the timed pass below gathers and uploads again
        t1 = time.perf_counter(); sweep._stack_raw(mine, ctx); t_stack = time.perf_counter() - t1     # (untimed pass: the host gather alone)
    else:
        t_stack = 0.0
    comm.barrier()
    t0 = time.perf_counter()
    # data4sysid structs -> one block per quantity (host threads) -> upload (beside the seam test of the time vectors) -> passes
    tab = sweep.rand_models_sweep_batched(mine, ctx) if mine else {}
    t_local = time.perf_counter() - t0
    local = {i: {mt: tab[mt][:, k] for mt in tab} for k, i in enumerate(ids)}
    allres = sweep.gather_results(local, n_systems, comm)
    comm.barrier()
    dt = kc.max_over_ranks(comm, time.perf_counter() - t0)
    lin = np.stack([r["linear"] for r in allres], axis=1)
    mean, _ = sweep.sweep_statistics(lin)
    return {"systems": n_systems, "distinct_systems": True, "seconds": dt, "systems_per_s": n_systems / dt, "n_gpus": comm.world,
            "rank0_compute_seconds": t_local, "rank0_host_gather_seconds_alone": t_stack,
            "fits_per_system": int(sum(v.shape[0] for v in tab.values())) if tab else 23,
            "_gram": dict(ctx.__dict__.get("_sweep_gram", {})),
            "mean_linear_error_deg1_deg13": [float(mean[0]), float(mean[-1])],
            "workload": "evaluate_rand_models.m on 1024 generated 1-D random systems (Rsys restatement), 23 fits + validation "
                        "rollouts each, 128-system chunks round-robin over the ranks (BASELINE configs[4])"}


def bench_arm_closed_loop(ctx, kra):
    """BASELINE configs[2] as named: bilinear Kmpc, horizon 10, closed loop on the block-M reference with the arm model
    identified from the shipped 3-link data (poly-3, dim_red: N = 34), example_control.m settings, the identified
    model as the plant (Kmpc.run_simulation, Kmpc.m:403-512).  Fixtures: tests/golden (data files of the reference)."""
    gd = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(gd, "arm_data.npz")); ref = np.load(os.path.join(gd, "blockM_ref.npz"))["y"]
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    t0 = time.perf_counter()
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()
    t_sysid = time.perf_counter() - t0
    for _ in range(3):
        ks.get_Koopman(ks.snapshotPairs)
    tg = []
    for _ in range(15):
        t1 = time.perf_counter(); ks.get_Koopman(ks.snapshotPairs); tg.append(time.perf_counter() - t1)
    mpc = kra.Kmpc(ks, horizon=10, input_bounds=[-7 * np.pi / 8, 7 * np.pi / 8], input_slopeConst=1e-1, input_smoothConst=None,
                   state_bounds=None, cost_running=10, cost_terminal=100, cost_input=0.1 * np.array([3e-2, 2e-2, 1e-2]),
                   projmtx=ks.model["C"][-2:, :])
    mpc.run_simulation(ref[:20])
    t0 = time.perf_counter()
    res = mpc.run_simulation(ref)
    dt = time.perf_counter() - t0
    n = len(res["comp_time"])
    proj = ks.model["C"][-2:, :6]
    err = float(np.mean(np.linalg.norm(res["Y"][1:] @ proj.T - res["R"][1:], axis=1)))
    return {"steps": n, "steps_per_s": n / dt, "controller_us_per_step": float(np.median(res["comp_time"])) * 1e6, "N": int(ks.params["N"]),
            "mean_tracking_error": err, "sysid_seconds": t_sysid,
            "get_koopman_end_to_end_ms": float(np.median(tg)) * 1e3, "get_koopman_pairs": int(ks.snapshotPairs["alpha"].shape[0]),
            "get_koopman_W": int(ks.basis_dev.W),
            "reference_recorded": "MATLAB R2019a stored comp_time of the same controller shape: median 8.7 ms/step",
            "workload": "bilinear Kmpc horizon 10 on the block-M reference, arm model N=34 (poly-3, dim_red) from the shipped "
                        "3-link data, model as plant (BASELINE configs[2])"}


def roofline_block(kernel, exec_flop, dense_flop, ms, note=None, **extra):
    """One kernel's line: `achieved` / `frac` count what the kernel EXECUTES on the matrix pipe (MFMA instructions x 512 flop,
    padding included) - never above 1; the dense-equivalent figure (SURVEY 8(d)'s per-unit count of the products the reference
    forms) stands beside it."""
    t = ms * 1e-3
    out = {"kernel": kernel, "bound": "mfma", "ms": ms, "achieved": exec_flop / t / 1e12, "peak": PEAK_F64_MFMA_TFLOPS, "unit": "TFLOP/s",
           "frac": exec_flop / t / 1e12 / PEAK_F64_MFMA_TFLOPS, "executed_flop_per_launch": exec_flop,
           "dense_equivalent_flop_per_launch": dense_flop, "dense_equivalent_achieved": dense_flop / t / 1e12,
           "dense_equivalent_frac": dense_flop / t / 1e12 / PEAK_F64_MFMA_TFLOPS}
    if note:
        out["note"] = note
    out.update(extra)
    return out


def bench_get_koopman(ctx, kra, Ns):
    """The drop-in call end to end: `koopData = Ksysid.get_Koopman(snapshotPairs)` (Ksysid.m:987-1092) through the host
    mirror - host arrays in (pageable numpy, as MATLAB hands mxArrays over), koopData with K on the host out: refill of the
    resident snapshot object + fused Gram + solve + K fetch.  koopData.Px / .Py (:1085-1086) are materialised on first
    access; what that costs is timed separately.  Config 2's shape (bilinear poly-3, W = 336) on a synthetic trial."""
    rng = np.random.default_rng(11)
    T = Ns + 1
    y = np.cumsum(rng.standard_normal((T, 6)), axis=0) * 0.01
    y = np.tanh(y + 0.3 * rng.standard_normal((T, 6)))
    u = rng.uniform(-1, 1, (T, 3))
    t = np.arange(T) * 0.01
    trial = {"t": t, "y": y, "u": u}
    val = {"t": t[:400], "y": y[:400], "u": u[:400]}
    ks = kra.Ksysid({"train": [trial], "val": [val]}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=False)
    sp = ks.snapshotPairs
    for _ in range(3):
        ks.get_Koopman(sp)
    ts = []
    for _ in range(15):
        t1 = time.perf_counter(); kd = ks.get_Koopman(sp); ts.append(time.perf_counter() - t1)
    t1 = time.perf_counter(); px = kd["Px"]; py = kd["Py"]; t_pxpy = time.perf_counter() - t1
    kd = ks.get_Koopman(sp)
    t1 = time.perf_counter(); px = kd["Px"]; py = kd["Py"]; t_pxpy = min(t_pxpy, time.perf_counter() - t1)
    return {"get_koopman_end_to_end_ms": float(np.median(ts)) * 1e3, "pairs": int(sp["alpha"].shape[0]), "W": int(ks.basis_dev.W),
            "PxPy_on_first_access_ms": t_pxpy * 1e3, "PxPy_bytes": int(px.nbytes + py.nbytes),
            "note": "host arrays in -> koopData (K on the host) out, through Ksysid.get_Koopman of the host mirror; Px/Py = the econ "
                    "lift (N columns), materialised lazily"}


def bench_width_points(ctx, kra, Ns):
    """SURVEY 8(d)'s other fit shapes next to W = 336 - W = 200 (N = 50: the first 49 poly-3 rows + constant) and W = 136
    (N = 34: econ lift through a pcs matrix, the shape of example_sysid.m with dim_red) - and two non-polynomial
    dictionaries (def_fourierLift Ksysid.m:694-731, def_gaussianLift :790-817).  Kernel time of the fused lift+Gram launch
    measured like the headline's: mean HIP-event duration over a queue of pipelined fits (a lone synchronous launch after an
    idle stretch runs at a lower clock, profiles/r02_gram_launch_durations.txt)."""
    out = {}
    a, b, u = synth_pairs(Ns, seed=5)
    snaps = kra.Snapshots(ctx, a, b, u)
    a3, b3, u3 = synth_pairs(Ns, 3, 3, seed=6)
    snaps3 = kra.Snapshots(ctx, a3, b3, u3)
    tab = kra.poly_exponent_table(6, 3)
    rng = np.random.default_rng(3)
    pcs = np.linalg.qr(rng.standard_normal((84, 27)))[0]
    centres = rng.uniform(-1, 1, (6, 20))
    shapes = [("W200", kra.Basis(ctx, "bilinear", 6, 3, [("poly", tab[6:49])]), snaps, "kp_gram3_kernel<6,3,false,false,false,true>"),
              ("W136_pcs", kra.Basis(ctx, "bilinear", 6, 3, [("poly", tab[6:])], pcs), snaps, "kp_gram3_prelift_mfma_kernel + kp_gram3_kernel<.,3,false,false,true>"),
              ("fourier1_nzeta3", kra.Basis(ctx, "bilinear", 3, 3, [("fourier", 1)]), snaps3, "kp_gram3_prelift_ext_kernel + kp_gram3_kernel<.,3,false,false,true>"),
              ("gaussian20", kra.Basis(ctx, "bilinear", 6, 3, [("gaussian", centres)]), snaps, "kp_gram3_prelift_ext_kernel + kp_gram3_kernel<.,3,false,false,true>")]
    if os.environ.get("KP_BENCH_MORE_WIDTHS"):    # same width without the projection: what the econ lift costs
        shapes.append(("W136_plain", kra.Basis(ctx, "bilinear", 6, 3, [("poly", tab[6:33])]), snaps, "kp_gram3_kernel"))
    for name, basis, sn, kern in shapes:
        W = basis.W
        for _ in range(48):                        # untimed queue: kernel variants loaded, clock up
            kra.fit(ctx, basis, sn, fetch=False)
        ctx.synchronize()
        for _ in range(64):
            kra.fit(ctx, basis, sn, fetch=False)
        ctx.synchronize()
        ms, n_l, ex = ctx.timer(0), int(ctx.timer(7)), ctx.timer(10)
        F_ = W * (W + 1) + 2.0 * W * W
        out[name] = {"W": W, "N": basis.N, "gram_ms": ms, "launches_averaged": n_l, "pairs_per_s_gram_only": Ns / (ms * 1e-3),
                     "roofline": roofline_block(kern or "fused lift+Gram (see DESIGN 3.1 for the variant)", ex * Ns, F_ * Ns, ms)}
        basis.close()
    snaps.close(); snaps3.close()
    return out


def bench_wide_points(ctx, kra):
    """Dictionaries beyond one workgroup's reach (round 5): `def_fourierLift` with degree 1 on the arm's six
    states (Ksysid.m:694-731: 728 functions; linear row W = 738, bilinear row W = 2 940) at the shipped data set's 11 999 pairs
    and at 1e5.  Grams: lifted panels in HBM + TN products on the matrix pipe (csrc/kp_wide.hip); K = Px \\ Py: blocked Cholesky /
    substitution over all CUs (csrc/kp_fit.hip).  Synchronous fits (the pipelined queue serves W <= 512)."""
    out = {}
    for mt in ("linear", "bilinear"):
        basis = kra.Basis(ctx, mt, 6, 3, [("fourier", 1)])
        W = basis.W
        F_ = W * (W + 1) + 2.0 * W * W
        for Ns in (11999, 100000):
            a, b, u = synth_pairs(Ns, seed=11)
            sn = kra.Snapshots(ctx, a, b, u)
            kra.fit(ctx, basis, sn, fetch=False)
            reps = 3
            t0 = time.perf_counter()
            for _ in range(reps):
                kra.fit(ctx, basis, sn, fetch=False)
            dt = (time.perf_counter() - t0) / reps
            gram_ms, solve_ms, ex = ctx.timer(0), ctx.timer(1), ctx.timer(10)
            out[f"{mt}_W{W}_Ns{Ns}"] = {"W": W, "snapshots": Ns, "ms_per_fit": dt * 1e3, "pairs_per_s": Ns / dt, "gram_ms": gram_ms, "solve_ms": solve_ms,
                                        "rank": ctx.last_rank(),
                                        "roofline": roofline_block("kp_lift_kernel + kp_tn_gemm_kernel<8,6|4> (upper tiles of Px'Px, Px'Py; bilinear rows: 10 weighted products each of the psi panel)", ex * Ns, F_ * Ns, gram_ms,
                                                                   note="gram_ms includes the lift of the panel (fourier: 6 sincos per function and snapshot)"),
                                        "solve_flop": W ** 3 / 3.0 + 2.0 * W ** 3, "solve_tflops": (W ** 3 / 3.0 + 2.0 * W ** 3) / (solve_ms * 1e-3) / 1e12}
            sn.close()
        basis.close()
    return out


def bench_rank_deficient(ctx, kra):
    """MATLAB's `\\` on the arm data WITHOUT dim_red (Ksysid.m:1069; bilinear poly-3: rank 252 of 336): the plain
    factorisation stops at its first rounding-level pivot, the blocked pivoted Cholesky over many workgroups selects the
    column subset, its factor serves the substitution.  One synchronous fit on the shipped data set (tests/golden)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "arm_data.npz"))
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    data = {"train": train, "val": [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]}
    import warnings
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for mt, deg in (("bilinear", 3), ("linear", 3)):
            ks = kra.Ksysid(data, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[deg], snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=False)
            sp = ks.snapshotPairs
            sn = ks._resident_snapshots(sp["alpha"], sp["beta"], sp["u"])
            for _ in range(5):
                kra.fit(ctx, ks.basis_dev, sn)
            t0 = time.perf_counter()
            for _ in range(30):
                kra.fit(ctx, ks.basis_dev, sn)
            dt = (time.perf_counter() - t0) / 30
            out[f"{mt}_poly{deg}"] = {"W": ks.basis_dev.W, "rank": ctx.last_rank(), "snapshots": int(sp["alpha"].shape[0]), "ms_per_fit": dt * 1e3,
                                      "gram_ms": ctx.timer(0)}
    return out


def bench_ns_points(ctx, kra, basis, sizes=(11999, 1000000, 10000000)):
    """SURVEY 8(d)'s other snapshot counts on the headline dictionary (W = 336): 11 999 (the shipped arm data set), 1e6
    and 1e7 pairs per fit, all resident in HBM (1.2 GB at 1e7).  Same measurement as the headline: a queue of pipelined fits,
    kernel time = mean HIP-event duration of the fused lift+Gram launch, wall time per fit over the queue."""
    out = {}
    W = basis.W
    F_ = W * (W + 1) + 2.0 * W * W
    for Ns in sizes:
        a, b, u = synth_pairs(Ns, seed=9)
        sn = kra.Snapshots(ctx, a, b, u)
        del a, b, u
        n_q = int(max(8, min(64, 4e7 // Ns)))
        for _ in range(n_q):
            kra.fit(ctx, basis, sn, fetch=False)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_q):
            kra.fit(ctx, basis, sn, fetch=False)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / n_q
        ms, n_l, ex = ctx.timer(0), int(ctx.timer(7)), ctx.timer(10)
        out[f"Ns{Ns}"] = {"snapshots": Ns, "fits_queued": n_q, "ms_per_fit": dt * 1e3, "pairs_per_s": Ns / dt, "gram_ms": ms,
                          "launches_averaged": n_l, "roofline": roofline_block("fused lift+Gram, W=336", ex * Ns, F_ * Ns, ms)}
        sn.close()
    return out


def cpu_baseline_mpc(pack):
    """The oracle's literal Kmpc step (Bhat from dense matrix powers, 4 rebuilds folded into one,
    exact active-set QP) on the host, on a bounded sample of the same problems."""
    from oracle import koopman_oracle as ko
    setup, N, zeta, u_prev, Yr = pack
    dic = ko.build_dictionary("bilinear", 6, 3, ["poly"], [3])
    s = ko.MpcSetup("bilinear", setup["A"], setup["B"], 3, setup["Np"], setup["proj"], setup["q_run"], setup["q_term"], setup["r"],
                    np.stack([setup["lo"], setup["hi"]], axis=1), setup["slope"], None, None, 6)
    t0 = time.perf_counter(); n = 0
    for i in range(len(zeta)):
        z = ko.econ_full(dic, zeta[i][None, :])[0]
        ko.mpc_step(s, z, u_prev[i], Yr[i].reshape(-1, 2))
        n += 1
        if time.perf_counter() - t0 > 10.0:
            break
    dt = (time.perf_counter() - t0) / n
    return {"value": 1.0 / dt, "unit": "MPC steps/s", "cores": 1, "kind": "port",
            "sample": f"{n} literal Kmpc steps (numpy), N={N}, {dt*1e3:.1f} ms each"}


def one_caller_main(args):
    """ONE process, ONE calling thread, `--gpus` devices through the kp_multi_* entry points (the reference's host shape: a
    single MATLAB interpreter, Ksim.m:147 / evaluate_rand_models.m:45 - no second process, no RCCL): the lasso grid of
    configs[3], the random-system sweep of configs[4], a batch of MPC problems and one fit sharded over snapshots.  Prints one
    JSON object.  KP_ONE_CALLER_IDS=0,0 lists devices explicitly (the same device twice on a one-GPU box)."""
    ids = [int(x) for x in os.environ["KP_ONE_CALLER_IDS"].split(",")] if os.environ.get("KP_ONE_CALLER_IDS") else list(range(args.gpus))
    n_gen = max(1, args.rand_systems // RAND_CHUNK)               # the SAME distinct systems as the per-process block (seeded per chunk)
    chunks = gen_rand_systems(list(range(n_gen)))                 # host, before the GPUs are touched
    import koopman_realizations_amd as kra
    from koopman_realizations_amd import sweep
    from koopman_realizations_amd.multi import Multi, MultiMpc
    res = {"device_ids": ids, "host": "one process, one calling thread; a library-owned worker thread + context per device"}
    mg = Multi(ids)
    Ns = args.snapshots
    a, b, u = (np.asfortranarray(x) for x in synth_pairs(Ns, seed=0))
    exps = kra.poly_exponent_table(6, 3)[6:]
    dic = ("bilinear", 6, 3, [("poly", exps)], None)
    N, W = 84, 336

    def best(fn, reps=3):
        ts = []
        for _ in range(reps):
            t1 = time.perf_counter(); r = fn(); ts.append(time.perf_counter() - t1)
        return min(ts), r
    # (a) configs[3]: 64 lasso values on ONE snapshot matrix, value i on device i mod n; K stack into a page-locked block
    vals = np.geomspace(1e-2, 1e2, 64)
    out = mg.host_array("Kgrid", (64, W, W))
    mg.fit(dic, a, b, u, vals, out=out)                           # every buffer at its final size, dictionaries resident
    dt, Ks = best(lambda: mg.fit(dic, a, b, u, vals, out=out))
    tm = mg.timers()
    l1 = np.abs(Ks).sum(axis=(1, 2))
    res["lasso_grid"] = {"values": 64, "seconds": dt, "values_per_s": 64 / dt, "W": W, "n_devices": len(ids),
                         "per_device_ms": {"upload": tm[:, 0].tolist(), "device": tm[:, 1].tolist(), "gather": tm[:, 2].tolist(), "job": tm[:, 3].tolist()},
                         "budget_met": bool(np.all(l1 <= vals * N * (1 + 1e-9) + 1e-12)),
                         "gather": "each device DMAs its own K matrices into the caller's page-locked stack (no all-gather)",
                         "note": "host data in, K stack on the host out; device 0 uploads the 12 MB snapshot matrix and forms the Grams once, "
                                 "the other devices receive [G | C] (1.8 MB) by a peer copy and only factorise / solve their values"}
    # (b) ONE fit sharded over snapshots: rows dealt over the devices, [G | C] to device 0 by peer copy, one solve
    sh = {}
    for Ns_tot in (Ns, 10000000):
        try:
            a2, b2, u2 = (a, b, u) if Ns_tot == Ns else (np.asfortranarray(x) for x in synth_pairs(Ns_tot, seed=3))
            mg.fit_sharded(dic, a2, b2, u2)
            dts, Ksh = best(lambda: mg.fit_sharded(dic, a2, b2, u2), reps=3 if Ns_tot <= 1000000 else 2)
            tm = mg.timers()
            sh[f"Ns{Ns_tot}"] = {"snapshots_total": Ns_tot, "ms_per_fit": dts * 1e3, "pairs_per_s": Ns_tot / dts,
                                 "per_device_ms": {"upload": tm[:, 0].tolist(), "gram": tm[:, 1].tolist(), "exchange": tm[:, 2].tolist()},
                                 "note": "host arrays in (PCIe upload of every device's rows inside the time), K on the host out"}
            if Ns_tot == Ns:
                Kls = Ksh[0].T
        except Exception as e:
            sh[f"Ns{Ns_tot}"] = {"error": repr(e)[:300]}
    res["snapshot_sharded_fit"] = dict(sh, exchange="peer copy of 2 W^2 doubles per device to device 0 (xGMI), summed in device order", scaling="strong")
    # (c) configs[4]: 1024 random systems, contiguous chunks per device, three nested passes
    mine = [s_ for c in sorted(chunks) for s_ in chunks[c]]
    Y, U, k, Yv, Uv = sweep._stack_raw(mine)
    Y, U, Yv, Uv = (np.ascontiguousarray(x) for x in (Y, U, Yv, Uv))
    nsys = Y.shape[0]
    dicts = {mt: (mt, 1, 1, [("poly", kra.poly_exponent_table(1 + (mt == "nonlinear"), D)[1 + (mt == "nonlinear"):])], None)
             for mt, D in sweep.MAX_DEGREE.items()}

    def run_sweep():
        tr = mg.traj_upload(Y, U, k, Yv, Uv)
        t_up = mg.timers()[:, 0].tolist()
        errs, t_dev = {}, {}
        for mt, D in sweep.MAX_DEGREE.items():
            e, st = tr.sweep_eval_nested(dicts[mt], D, 4.0 if mt == "nonlinear" else np.inf)
            errs[mt] = np.where(st != 0, np.nan, e[:, :, 0]); t_dev[mt] = mg.timers()[:, 1].tolist()
        tr.close()
        return errs, t_up, t_dev
    run_sweep()
    dtw, (errs, t_up, t_dev) = best(run_sweep)
    mean, _ = sweep.sweep_statistics(errs["linear"])
    res["rand_sweep"] = {"systems": nsys, "distinct_systems": int(n_gen * RAND_CHUNK), "seconds": dtw, "systems_per_s": nsys / dtw, "n_devices": len(ids),
                         "per_device_ms": {"upload": t_up, "passes": t_dev}, "mean_linear_error_deg1_deg13": [float(mean[0]), float(mean[-1])],
                         "note": f"{nsys} distinct generated systems (the population of the per-process block); stacked raw trials in (host "
                                 "gather of the data4sysid structs excluded), error tables out"}
    # (d) batched MPC: 4096 problems per device
    A = np.asfortranarray(Kls[:N, :N].T); B = np.asfortranarray(Kls[N:, :N].T)
    proj = np.zeros((2, N)); proj[0, 4] = proj[1, 5] = 1.0
    u_fac = 2.8
    mm = MultiMpc(mg, "bilinear", A, B, 10, proj, 10.0, 100.0, 0.1 * np.array([3e-2, 2e-2, 1e-2]), np.full(3, -7 * np.pi / 8 / u_fac),
                  np.full(3, 7 * np.pi / 8 / u_fac), 1e-1 * u_fac)
    nb = args.mpc_batch * len(ids)
    zeta, u_prev, Yr = mpc_inputs(nb)
    ctx0 = kra.Context(ids[0])
    bs = kra.Basis(ctx0, "bilinear", 6, 3, [("poly", exps)])
    from koopman_realizations_amd import _ffi as F
    Z = np.ascontiguousarray(bs.lift(F.LIFT_ECON, zeta))
    bs.close(); ctx0.close()
    mm.step_batch(Z, u_prev, Yr)
    dtb, (Ub, stb) = best(lambda: mm.step_batch(Z, u_prev, Yr))
    res["mpc_batch"] = {"problems": nb, "seconds": dtb, "problems_per_s": nb / dtb, "solved": int((stb == 0).sum()), "n_devices": len(ids),
                        "per_device_ms": mg.timers()[:, 1].tolist()}
    mm.close()
    mg.close()
    print(json.dumps(res), flush=True)


def run_one_caller(args, n_dev, timeout=240.0):
    """The one-caller block in a FRESH process (started by rank 0 when its own sections are done): a failure or a hang there
    costs this block, never the line."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--one-caller", "--gpus", str(n_dev), "--snapshots", str(args.snapshots),
           "--mpc-batch", str(args.mpc_batch), "--rand-systems", str(args.rand_systems)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "KP_FORCE_DEVICE")}
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode == 0 and lines:
            return json.loads(lines[-1])
        return {"error": f"rc {r.returncode}: " + (r.stderr or r.stdout)[-400:]}
    except Exception as e:
        return {"error": repr(e)[:300]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--snapshots", type=int, default=100000)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-mpc", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the lasso-grid, random-sweep and width-point sections")
    ap.add_argument("--mpc-steps", type=int, default=300)
    ap.add_argument("--mpc-batch", type=int, default=4096)
    ap.add_argument("--rand-systems", type=int, default=1024)
    ap.add_argument("--one-caller", action="store_true", help="(internal) the single-process multi-GPU block: kp_multi_* over --gpus devices")
    ap.add_argument("--no-one-caller", action="store_true")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned (K, float64) as DIR/K.npy, for output-for-output comparison of builds")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.one_caller:
        one_caller_main(args)
        return

    from koopman_realizations_amd import comm as kc
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # launched directly: one fresh process per GPU, started before anything here has touched a GPU
        out = kc.spawn_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], args.gpus)
        lines = [l for l in out.splitlines() if l.startswith("{")]
        print(lines[-1] if lines else out)
        return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    extras_on = not args.no_extras and args.degree == 3
    # host-side generation of this rank's share of the random systems (worker processes, before the GPU is touched)
    n_chunks = max(1, args.rand_systems // RAND_CHUNK)
    chunks = gen_rand_systems([c for c in range(n_chunks) if c % world == rank]) if extras_on else {}

    # the generated systems are ~35k long-lived Python objects: keep the cyclic collector from walking them inside the timed
    # regions (a generation-2 pass costs milliseconds and lands wherever the allocation counter trips)
    import gc
    gc.collect()
    gc.freeze()
    if chunks:
        time.sleep(0.5)                            # let the generator's worker processes be reaped before the launch-rate-bound region
    import koopman_realizations_amd as kra
    ctx, comm = kc.init_from_env(kra.Context)      # one process per GPU; RCCL communicator through the C ABI when world > 1
    Ns = args.snapshots
    alpha, beta, u = (np.asfortranarray(x) for x in synth_pairs(Ns, seed=rank))   # column-major, the layout MATLAB hands over
    basis = kra.Basis(ctx, "bilinear", 6, 3, [("poly", kra.poly_exponent_table(6, args.degree)[6:])])
    t_up = []
    for _ in range(7):                              # the first two also allocate the two halves of the pinned staging ring
        t1 = time.perf_counter(); snaps = kra.Snapshots(ctx, alpha, beta, u); t_up.append(time.perf_counter() - t1)
        snaps.close()
    snaps = kra.Snapshots(ctx, alpha, beta, u)      # resident in HBM before timing
    W = basis.W
    ctx.fit_async_slots(max(args.steps, args.warmup, 1))   # every K of the timed region stays retrievable

    # Steps are independent fits (the unit of the reference's sweeps), issued through the library's asynchronous pipeline:
    # the solve of fit i (second HIP stream) overlaps the fused Gram kernel of fit i+1; each K lands in its own slot of
    # the device result ring; everything is drained and the ranks' last K matrices are gathered (RCCL, device to
    # device) inside the timed region.
    # one queue as deep as the timed region's first (at least one full batch of deferred solves): every buffer of the pipeline
    # and of the HIP runtime (kernel-argument and signal pools grow with the queue depth) at its final size, every kernel
    # variant loaded (not counted as warm-up)
    # ... and the device at its sustained clock: the first ~60 Gram launches after an idle or lightly loaded stretch run
    # 470 -> 405 us (profiles/r02_gram_launch_durations.txt), so the queue is 256 fits (110 ms) deep
    for _ in range(max(256, args.steps)):
        kra.fit(ctx, basis, snaps, fetch=False)
    ctx.synchronize()
    for _ in range(args.warmup):
        kra.fit(ctx, basis, snaps, fetch=False)
    ctx.synchronize()
    if world > 1:
        comm.all_gather_fit(args.warmup - 1 if args.warmup else 0, W) if args.warmup else None
    # the synchronisation above ended with the warm-up's few one-workgroup factorisations: 0.3 ms of a nearly idle device,
    # after which the Gram kernel needs ~20 launches to come back from 420 to 405 us (same file).  A short queue of Gram
    # launches alone (no solves) leaves only the host's own latency between the last busy kernel and the timed region.
    for _ in range(32):
        kra.fit_gram(ctx, basis, snaps, fetch=False)
    ctx.synchronize()
    comm.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        kra.fit(ctx, basis, snaps, fetch=False)     # enqueue: Gram on stream 1, solve on stream 2
    t_enq = time.perf_counter() - t0                # host time to enqueue all fits (the device drains behind it)
    ctx.synchronize()                               # all fits complete
    Kall = comm.all_gather_fit(args.steps - 1, W) if world > 1 else None    # the sweep's only collective: final gather
    comm.barrier()
    dt = kc.max_over_ranks(comm, time.perf_counter() - t0)
    # timer 0 = mean HIP-event duration of the last min(steps, 64) Gram launches of the timed region (timer 7 = count)
    g_ms, red_ms, solve_ms, n_timed = ctx.timer(0), ctx.timer(6), ctx.timer(1), int(ctx.timer(7))
    exec_pair_head = ctx.timer(10)          # flop per pair this kernel executes on the matrix pipe (padding included)
    # every K of the timed region is retrievable and they all solve the same system
    K_first, K_last = ctx.fit_result(0, W), ctx.fit_result(args.steps - 1, W)
    k_spread = float(np.abs(K_first - K_last).max())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"K": K_last})
    # ... and what bringing ALL of them to the host costs (a sweep that keeps every K): page-locked destination, direct DMA
    n_f = min(args.steps, 64)
    ctx.fit_results(0, n_f, W)
    t1 = time.perf_counter(); Kst = ctx.fit_results(0, n_f, W); k_fetch_us = (time.perf_counter() - t1) / n_f * 1e6
    assert np.array_equal(Kst[0].T, K_first)

    # one-fit latency (no overlap): synchronous path of the same entry point
    os.environ["KP_NO_ASYNC"] = "1"
    lat = []
    for _ in range(5):
        t1 = time.perf_counter(); kra.fit(ctx, basis, snaps, fetch=False); lat.append(time.perf_counter() - t1)
    del os.environ["KP_NO_ASYNC"]
    fit_latency_ms = float(np.median(lat)) * 1e3
    # the public entry point end to end: Ksysid.get_Koopman's device part with K fetched (one refinement step excluded)
    kra.fit(ctx, basis, snaps)
    t1 = time.perf_counter(); kra.fit(ctx, basis, snaps); fit_fetch_ms = (time.perf_counter() - t1) * 1e3

    # fits whose snapshot matrix arrives from HOST memory every time (a caller that hands each get_Koopman call new
    # data): two device objects refilled alternately through the pinned staging ring (kp_snapshots_update), the
    # transfer of one overlapping the Gram kernel of the other.  Reported beside `value`, never part of it.
    streamed_ms = None
    if rank == 0 and world == 1:
        ring2 = [snaps, kra.Snapshots(ctx, alpha, beta, u)]
        n_st = 64
        for rep in range(3):                        # the last pass counts (the section above left the device lightly loaded)
            t1 = time.perf_counter()
            for i in range(n_st):
                ring2[i % 2].update(alpha, beta, u)
                kra.fit(ctx, basis, ring2[i % 2], fetch=False)
            ctx.synchronize()
            streamed_ms = (time.perf_counter() - t1) / n_st * 1e3
        ring2[1].close()

    mpc_res = arm_res = widths = ns_pts = wide_pts = rankdef = None
    if rank == 0 and not args.no_mpc and world == 1:     # latency-bound sections only in the single-GPU run
        mpc_res = bench_mpc(ctx, kra, basis, snaps, args)
        arm_res = bench_arm_closed_loop(ctx, kra)
    gk_res = None
    if rank == 0 and extras_on and world == 1:
        widths = bench_width_points(ctx, kra, Ns)
        ns_pts = bench_ns_points(ctx, kra, basis) if (Ns == 100000 and args.degree == 3) else None
        gk_res = bench_get_koopman(ctx, kra, Ns)
        wide_pts = bench_wide_points(ctx, kra)
        rankdef = bench_rank_deficient(ctx, kra)
    lasso_res = sweep_res = shard_res = None
    if extras_on and world > 1:
        # SURVEY 8(e) pattern 2: ONE fit whose snapshots are sharded over the ranks (strong scaling: the total is fixed) - local
        # Gram kernel, one all-reduce of [G | C] (1.8 MB) on the device, the same solve on every rank.  Needs the RCCL
        # communicator (without one kp_fit_sharded is the local fit and the block says so).
        shard_res = {}
        for Ns_tot in (100000, 10000000):
            try:
                per = Ns_tot // world
                a_s, b_s, u_s = synth_pairs(per, seed=100 + rank)
                sn_s = kra.Snapshots(ctx, a_s, b_s, u_s)
                del a_s, b_s, u_s
                n_q = 16 if Ns_tot <= 1000000 else 4
                for _ in range(3):
                    kra.fit_sharded(ctx, basis, sn_s)
                comm.barrier()
                t1 = time.perf_counter()
                for _ in range(n_q):
                    kra.fit_sharded(ctx, basis, sn_s)
                comm.barrier()
                dt_s = kc.max_over_ranks(comm, (time.perf_counter() - t1) / n_q)
                sn_s.close()
                shard_res[f"Ns{Ns_tot}"] = {"snapshots_total": per * world, "ms_per_fit": dt_s * 1e3, "pairs_per_s": per * world / dt_s,
                                             "exchange": "one all-reduce of 2 W^2 doubles (RCCL, device to device)" if comm.kind == "rccl"
                                             else f"none: comm is '{comm.kind}', every rank fitted its own shard only"}
            except Exception as e:                      # never let this section take the line down
                shard_res[f"Ns{Ns_tot}"] = {"error": repr(e)[:300]}
    if extras_on:                                        # sharded sections: every rank takes part
        # the grid belongs to ONE fit: every rank holds the same snapshot matrix (rank 0's) for this section
        snaps_l = snaps
        if rank != 0:
            a0, b0, u0 = synth_pairs(Ns, seed=0)
            snaps_l = kra.Snapshots(ctx, a0, b0, u0)
        lasso_res = bench_lasso(ctx, comm, kra, basis, snaps_l)
        if lasso_res is not None and comm.rank == 0:
            try:
                lasso_res["ill_conditioned"] = bench_lasso_ill_conditioned(ctx, kra)
            except Exception as e:                                                    # a secondary point never takes the line down
                lasso_res["ill_conditioned"] = {"error": str(e)}
        sweep_res = bench_rand_sweep(ctx, comm, kra, chunks, n_chunks * RAND_CHUNK)

    if rank == 0:
        flops_pair = W * (W + 1) + 2.0 * W * W                 # F(336) = 339 024, the dense products the reference forms
        # what the Kronecker kernel executes on the matrix pipe for the identical G, C (kp_timer_get 10: jobs x quads x weights
        # MFMA instructions per 4 snapshots, 512 flop each, padding included)
        exec_pair = exec_pair_head
        # HBM traffic of the dominant kernel: PMC counters are collected in separate rocprofv3 passes of this
        # same command (tools/prof_round.sh) and committed under profiles/; null when the workload differs
        traffic, prof_note = None, None
        for pj in ("r06_pmc_summary.json", "r05_pmc_summary.json", "r04_pmc_summary.json", "r03_pmc_summary.json", "r02_pmc_summary.json", "r01_pmc_summary.json"):
            pj = os.path.join(ROOT, "profiles", pj)
            if os.path.exists(pj) and Ns == 100000 and args.degree == 3:
                try:
                    pr = json.load(open(pj))
                    traffic = pr["gram_traffic_bytes_per_launch"]
                    prof_note = {"executed_flop_per_launch": pr["gram_executed_flop"], "mfma_busy_cycles_per_instr": pr["gram_mfma_busy_cycles_per_instr"],
                                 "source": "profiles/" + os.path.basename(pj)}
                    break
                except Exception:
                    pass
        upload_ms = float(np.median(t_up)) * 1e3
        res = {
            "metric": "EDMD snapshot-pairs/sec (bilinear fit, 3-link arm, poly-3)",
            "value": world * Ns * args.steps / dt,
            "unit": "snapshot-pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"bilinear Koopman fit, poly degree {args.degree}, {Ns} synthetic snapshot pairs per GPU, "
                                   f"N={basis.N}, W={W} (BASELINE configs[1])",
                       "snapshots_per_gpu": Ns, "W": W,
                       "parallelism": f"{world} rank(s), independent fits per rank, one RCCL all-gather of the K matrices at the end",
                       "comm": comm.kind + (f" (RCCL unavailable: {comm.fallback_reason})" if getattr(comm, "fallback_reason", "") else "")},
            "host_enqueue_ms_per_step": t_enq / args.steps * 1e3,
            "fit_latency_ms": fit_latency_ms, "fit_with_K_fetched_ms": fit_fetch_ms,
            "all_K_retrievable": True, "K_first_vs_last_max_abs_diff": k_spread, "K_fetch_us_per_fit_page_locked": k_fetch_us,
            "h2d": {"upload_ms": upload_ms, "pairs_per_s_upload_then_fit": Ns / ((upload_ms + dt / args.steps * 1e3) * 1e-3),
                    "streamed_ms_per_fit": streamed_ms,
                    "pairs_per_s_streamed_from_host": (Ns / (streamed_ms * 1e-3)) if streamed_ms else None,
                    "note": f"{15 * 8 * Ns / 1e6:.0f} MB of host snapshot pairs per fit over PCIe (pageable host arrays, staged through pinned "
                            "chunks); streamed = two device objects refilled alternately, transfer overlapping the other "
                            "object's Gram kernel; never part of `value`"},
            "kernel_ms": {"gram": g_ms, "gram_launches_averaged": n_timed, "gram_reduce": red_ms if red_ms > 0 else None, "solve": solve_ms},
            "untimed_prewarm_launches": {"pipelined_fits": max(256, args.steps), "gram_only": 32,
                                         "why": "clock ramp: the first ~60 Gram launches after an idle stretch run 470 -> 405 us "
                                                "(profiles/r02_gram_launch_durations.txt); `warmup` counts only the driver's W"},
            "roofline": dict(roofline_block("kp_gram3_kernel<6,3,false,false,false,true>", exec_pair * Ns, flops_pair * Ns, g_ms,
                                            note="frac = flop the kernel executes on the matrix pipe / mean kernel time of the timed region (HIP "
                                                 "events on the launch stream) / f64 matrix peak; dense_equivalent_* = SURVEY 8(d)'s W(W+1)+2W^2 "
                                                 "per pair (the Kronecker kernel produces the identical G, C with ~63% of those flop)"),
                             traffic=traffic, algorithmic_bytes_per_launch=120.0 * Ns,
                             hbm_algorithmic_GBs=120.0 * Ns / (g_ms * 1e-3) / 1e9, pmc=prof_note),
        }
        if mpc_res is not None:
            res["mpc"] = mpc_res
            res["mpc_arm_blockM"] = arm_res
        if widths is not None:
            res["width_points"] = widths
        if ns_pts is not None:
            res["snapshot_count_points"] = ns_pts
        if gk_res is not None:
            res["get_koopman"] = gk_res
        if wide_pts is not None:
            res["wide_dictionaries"] = wide_pts
        if rankdef is not None:
            res["rank_deficient_fit"] = rankdef
        if shard_res is not None:
            res["snapshot_sharded_fit"] = dict(shard_res, scaling="strong")
        if lasso_res is not None:
            res["lasso_grid"] = lasso_res
            res["rand_sweep"] = sweep_res
        # per-kernel rooflines of the secondary paths (the same fields as `roofline`; profiles/r03_*_kernel_stats.csv hold
        # the rocprofv3 rows of the same kernels)
        kern = []
        if widths is not None:
            kern += [dict(w["roofline"], point=k_) for k_, w in widths.items()]
        if ns_pts is not None:
            kern += [dict(w["roofline"], point="W336 " + k_) for k_, w in ns_pts.items()]
        if lasso_res is not None and lasso_res.get("_gemm"):
            g_ms_, g_cols = lasso_res.pop("_gemm")
            fl = 2.0 * W * W * g_cols
            Wp_ = -(-W // 112) * 112 if W == 336 else W          # row padding of the tile grid (none at W = 336)
            kern.append(dict(roofline_block("kp_symm_gemm2_kernel<7,.>", 2.0 * Wp_ * W * (-(-g_cols // 32) * 32), fl, g_ms_,
                                            note="first (widest) product G [K_1 .. K_nv] of the lasso grid's FISTA iteration"),
                             point=f"lasso product {W}x{W}x{int(g_cols)}"))
        if sweep_res is not None and sweep_res.get("_gram"):
            for mt, (ms_, W_, pairs, ex_) in sweep_res.pop("_gram").items():
                dense = (W_ * (W_ + 1) + 2.0 * W_ * W_) * pairs
                blk = roofline_block("kp_traj_gram_cols_kernel", (ex_ if ex_ > 0 else 1024.0) * pairs, dense, ms_,
                                     note="W <= 16: the upper triangle of G (10 blocks of 4 x 4) and C (16 blocks) on the matrix pipe, one "
                                          "v_mfma_f64_4x4x4_4b per block and 16 pairs (its four blocks take four pair groups), 8 operand reads "
                                          "per 26 MFMAs; 24 B per pair, so the pass is also priced against HBM")
                blk.update({"hbm_GBs": 24.0 * pairs / (ms_ * 1e-3) / 1e9, "hbm_frac": 24.0 * pairs / (ms_ * 1e-3) / 1e9 / PEAK_HBM_GBS})
                kern.append(dict(blk, point=f"rand sweep {mt} pass, W={W_}, {int(pairs)} pairs"))
        if lasso_res is not None:
            lasso_res.pop("_gemm", None)
        if sweep_res is not None:
            sweep_res.pop("_gram", None)
        if kern:
            res["kernels"] = kern
        if extras_on and not args.no_one_caller:
            # the reference's host shape: ONE process drives all `world` GPUs through kp_multi_* (fresh child process; the
            # other ranks of this launch idle meanwhile, waiting for the flag file below)
            res["one_caller"] = run_one_caller(args, world)
        if not args.no_cpu_baseline and world == 1:
            res["cpu_baseline"] = cpu_baseline(Ns, args.degree, seconds=6.0)
            if mpc_res is not None:
                res["cpu_baseline"]["mpc"] = cpu_baseline_mpc(mpc_res.pop("_setup"))
        if mpc_res is not None:
            mpc_res.pop("_setup", None)
        emit_result(res)
    # ranks other than 0 idle (no collective in flight: an RCCL barrier would spin on their GPUs) until rank 0 is through with
    # its host-only sections and the one-caller block, which uses every GPU of the launch
    flag = os.path.join("/tmp", f"kp_bench_done_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}")
    if world > 1:
        if rank == 0:
            open(flag, "w").close()
        else:
            t_w = time.perf_counter()
            while not os.path.exists(flag) and time.perf_counter() - t_w < 600.0:
                time.sleep(0.05)
    comm.barrier()
    if world > 1 and rank == 0:
        try:
            os.remove(flag)
        except OSError:
            pass
    ctx.close()


if __name__ == "__main__":
    main()
