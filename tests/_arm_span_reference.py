"""Host yardstick of the device arm plant: arm.ode45_span with the input / load row rules of include/koopman_hip_arm.h
(Arm.m's get_k for 'zoh' and 'interp', floor(t / Ts) for simulate_rampNhold).  Shared by the CPU and GPU arm tests."""
import numpy as np

from koopman_realizations_amd.arm import ode45_span


def golden_arm(golden, cls=None, **kw):
    import koopman_realizations_amd as kra
    gp = golden["arm_plant"]
    params = {k[2:]: (float(gp[k]) if gp[k].ndim == 0 else gp[k]) for k in gp.files if k.startswith("p_")}
    params.update(kw)
    return (cls or kra.Arm)(params, output_type="markers")


def get_k_row(t, s):
    """0-based row of u_in(get_k(s, t) + 1, :) (Arm.m:1004, 1044-1052): 1 at s = 0, j + 1 on (t_j, t_{j+1}]."""
    if s == 0:
        return 1
    return min(int(np.searchsorted(t, s, side="left")), t.size - 1)


def host_span(arm, t, u, w=None, rule="zoh", Ts=None, x0=None, rtol=1e-3, atol=1e-6):
    """One trial as the device's SPAN_* modes integrate it.  Returns (X, stats)."""
    t = np.asarray(t, dtype=np.float64).ravel()
    T = t.size
    w = np.zeros((T, 2)) if w is None else np.broadcast_to(np.asarray(w, dtype=np.float64), (T, 2))
    n = int(arm.params["Nlinks"])

    def f(s, x):
        if rule == "floor":
            q = np.floor(s / Ts)
            r = 0 if not q > 0 else min(int(q), T - 1)
            uu = u[r]
        else:
            r = get_k_row(t, s)
            uu = u[r]
            if rule == "interp":
                r1 = min(r + 1, T - 1)
                uu = u[r] + (u[r1] - u[r]) / (t[r1] - t[r]) * (s - t[r])        # Arm.m:1007
        return arm.vf(x, uu, tuple(w[r]))

    span = t[:-1] if rule == "interp" else t
    st = {}
    X = ode45_span(f, span, np.zeros(2 * n) if x0 is None else x0, rtol, atol, stats=st)
    return X, st
