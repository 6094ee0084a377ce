"""Test-side reference of the validation rollouts (csrc/kp_more.hip: kp_rollout): the host formula that picks the kernel's
regime, restated; the case table that walks every regime; a seeded model recipe whose trajectories neither decay nor grow;
and the plain recurrence of Ksysid.m:1285-1295 and 1678-1689 in np.longdouble.  Host only, numpy only.  Shared by
tests/test_rollout_reference.py (CPU: the table reaches the regimes it names, and the reference alone is far inside the
bound the device is held to) and tests/test_gpu_model_kernel_regimes.py; not collected by pytest."""
import functools

import numpy as np

# the constants of csrc/kp_more.hip (tests/test_rollout_reference.py reads the #defines and compares)
RO_STAGE = 8192            # doubles: A is staged in LDS when N * N <= RO_STAGE, B as well when both fit in 1.5 RO_STAGE
RO_TC = 256                # the longest chunk of time steps whose inputs and outputs are staged
LDS_BYTES = 128 * 1024     # the dynamic LDS the host code sizes the chunks for


def rollout_regime(N, m, bilinear, n_out):
    """(one_wave, stageA, stageB, tcmax) as kp_rollout's host code derives them."""
    mb = N * m if bilinear else m
    stageA = N * N <= RO_STAGE
    stageB = stageA and N * N + N * mb <= RO_STAGE + RO_STAGE // 2
    lds_model = (2 * N + (N * N if stageA else 0) + (N * mb if stageB else 0)) * 8
    tcmax = min(RO_TC, (LDS_BYTES - lds_model) // ((m + n_out) * 8))
    return N <= 64, bool(stageA), bool(stageB), int(tcmax)


# name -> (bilinear, N, m, n_out, T values, seed, regime (one_wave, stageA, stageB, tcmax), batched as well)
CASES = {
    "a": (False, 5, 1, 2, (1, 2, 255, 256, 257, 513), 101, (True, True, True, 256), True),
    "b": (False, 64, 3, 64, (1, 178, 179, 357), 102, (True, True, True, 178), False),       # one wave at its upper edge
    "c": (False, 65, 2, 6, (2, 256, 257), 103, (False, True, True, 256), False),            # 256 threads, staged
    "d": (True, 64, 3, 6, (2, 257), 104, (True, True, False, 256), True),                   # B not staged: 16384 > 12288
    "e": (True, 64, 2, 64, (60, 61, 121), 105, (True, True, True, 60), False),              # B staged exactly at its limit
    "f": (False, 90, 2, 90, (86, 87, 173), 106, (False, True, True, 86), False),            # the last staged N
    "g": (True, 91, 2, 91, (174, 175, 349), 107, (False, False, False, 174), True),         # the first unstaged N
    "h_lin": (False, 300, 1, 300, (52, 53, 105), 108, (False, False, False, 52), False),    # N > 256: the row loop wraps
    "h_bil": (True, 300, 1, 300, (52, 53, 105), 109, (False, False, False, 52), True),
    "i": (False, 7, 0, 7, (1, 300), 110, (True, True, True, 256), False),                   # m = 0: z+ = A z
}
BATCH = 5


def make_model(bilinear, N, m, T, seed):
    """A, B, z0, U of the recipe: Q an orthogonal factor of a Gaussian matrix; linear with inputs A = 0.95 Q, B = 0.1 randn;
    linear without inputs A = Q; bilinear A = Q, B = [B_1 ... B_m] with B_i = 0.05 R_i / ||R_i||_2; z0, U uniform in [-1, 1].
    (A bilinear model that decays has no affine term: its state goes to zero and the late chunks would test nothing.)"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
    if bilinear:
        A = Q
        blocks = []
        for _ in range(m):
            R = rng.standard_normal((N, N))
            blocks.append(0.05 * R / np.linalg.norm(R, 2))
        B = np.hstack(blocks) if blocks else np.zeros((N, 0))
    elif m > 0:
        A = 0.95 * Q
        B = 0.1 * rng.standard_normal((N, m))
    else:
        A = Q
        B = np.zeros((N, 0))
    z0 = rng.uniform(-1, 1, N)
    U = rng.uniform(-1, 1, (T, m))
    return A, B, z0, U


def rollout_reference(A, B, z0, U, bilinear, dtype=np.longdouble):
    """Z (T x N) with Z[0] = z0 and Z[t+1] = A Z[t] + B u_t (Ksysid.m:1678-1689), or A Z[t] + sum_i u_t[i] B_i Z[t] with
    B = [B_1 ... B_m] (:1285-1295), every operation in `dtype`."""
    A = np.asarray(A, dtype=dtype); B = np.asarray(B, dtype=dtype)
    U = np.asarray(U, dtype=dtype)
    T, m = U.shape
    N = A.shape[0]
    Z = np.empty((T, N), dtype=dtype)
    z = np.asarray(z0, dtype=dtype).copy()
    for t in range(T):
        Z[t] = z
        if t == T - 1:
            break
        zn = A @ z
        if bilinear:
            for i in range(m):
                zn = zn + (B[:, i * N:(i + 1) * N] @ z) * U[t, i]
        elif m > 0:
            zn = zn + B @ U[t]
        z = zn
    return Z


@functools.lru_cache(maxsize=None)
def case(name, T, index=0):
    """Model `index` of the case (index 0: the single call; 0 ... BATCH - 1: the members of its batch, all distinct) at length
    T, with its long-double trajectory; computed once and shared - do not modify."""
    bil, N, m, n_out, _, seed, _, _ = CASES[name]
    A, B, z0, U = make_model(bil, N, m, T, seed + 1000 * index)
    Z = rollout_reference(A, B, z0, U, bil)
    for a in (A, B, z0, U, Z):
        a.setflags(write=False)
    return {"bilinear": bil, "N": N, "m": m, "n_out": n_out, "A": A, "B": B, "z0": z0, "U": U, "Z": Z}
