"""CPU ORACLE -- test infrastructure only, never the product path.

The closed loop of the reference's demo (control.py:415-463) with a free
rigid-body plant, restated on tests/dynamics_oracle.py (`Tree`,
`controllaw_terms`, the arithmetics F64 / MP):

  bezier            Bezier.__call__ / eval_horner (control.py:30-46), operation for operation
  derivative        Bezier.derivative(1): control points degree (P[i+1] - P[i]), mult / (t_max - t_min)
  forward_dynamics  pin.aba as solve(crba, tau - nle)
  tick              desired state at the clamped clock, controllaw_terms, forward dynamics,
                    v += dt qdd then q += dt v (semi-implicit Euler), t += dt_traj
  rollout           `ticks` ticks, every one recorded

A curve is a tuple (points [n, dim], t_min, t_max, mult).  The clock t is a
float64 in every arithmetic and advances by one float64 add per tick, as the
reference's `tcur += DT`: the times the curves see are the same inputs for F64
and MP, so the 50-digit rollout is the truth FOR THOSE TIMES.
"""
from __future__ import annotations

import contextlib

import numpy as np

import dynamics_oracle as do


@contextlib.contextmanager
def keep_precision():
    """dynamics_oracle.arr rounds its argument to float64 first (its callers
    hand it float64 inputs).  A rollout feeds a tick's 50-digit state into the
    next tick, so while a tick runs, arrays already in the arithmetic pass
    through unrounded."""
    orig = do.arr

    def arr(ar, x):
        if ar.dtype is object and isinstance(x, np.ndarray) and x.dtype == object:
            return x
        return orig(ar, x)

    do.arr = arr
    try:
        yield
    finally:
        do.arr = orig


def bezier(ar, curve, t):
    """curve(t) in arithmetic ar; raises outside [t_min, t_max] as the reference."""
    P, t_min, t_max, mult = curve
    if not (t_min <= t <= t_max):
        raise ValueError("time out of range")
    P = do.arr(ar, P)
    n = len(P) - 1  # degree
    m = ar.num(mult)
    if n == 1:
        return m * P[0]
    u = (ar.num(t) - ar.num(t_min)) / (ar.num(t_max) - ar.num(t_min))
    uo, bc, tn = ar.num(1.0) - u, ar.num(1.0), ar.num(1.0)
    tmp = P[0] * uo
    for i in range(1, n):
        tn = tn * u
        bc = bc * (ar.num(float(n - i + 1)) / ar.num(float(i)))
        tmp = (tmp + (tn * bc) * P[i]) * uo
    return (tmp + (tn * u) * P[-1]) * m


def derivative(curve):
    """Bezier.derivative(1) in float64 (the control points the reference's maketraj hands on)."""
    P, t_min, t_max, mult = curve
    P = np.asarray(P, dtype=np.float64)
    n = len(P) - 1
    return n * (P[1:] - P[:-1]), t_min, t_max, mult * (1.0 / (t_max - t_min))


def clamp(curve, t):
    return min(max(t, curve[1]), curve[2])


def forward_dynamics(tree, q, v, tau, inverse=False):
    """qdd = M^-1 (tau - nle); inverse=True: the second formulation inv(M) @ rhs."""
    ar = tree.ar
    with keep_precision():
        M, b = do.crba(tree, q), do.nle(tree, q, v)
        rhs = do.arr(ar, tau) - b
    return ar.inv(M) @ rhs if inverse else ar.solve(M, rhs)


def tick(tree, q, v, t, cq, cv, dt_sim=1e-3, dt_traj=1e-2, euler="semi-implicit", **gains):
    """One tick -> (q, v, t, tau); q, v arrays of tree.ar, t float."""
    ar = tree.ar
    q_des, v_des = bezier(ar, cq, clamp(cq, t)), bezier(ar, cv, clamp(cv, t))
    with keep_precision():
        r = do.controllaw_terms(tree, q, v, q_des, v_des, **gains)
    rhs = r["tau"] - r["nle"]
    qdd = ar.solve(r["M"], rhs)
    dt = ar.num(dt_sim)
    v_new = v + dt * qdd
    q_new = q + dt * (v_new if euler == "semi-implicit" else v)
    return q_new, v_new, t + dt_traj, r["tau"]


def rollout(tree, q0, v0, t0, cq, cv, ticks, dt_sim=1e-3, dt_traj=1e-2, **gains):
    """-> dict(q, v, tau [ticks, nq] float64 (rounded from tree.ar), t [ticks])."""
    ar = tree.ar
    q, v, t = do.arr(ar, q0), do.arr(ar, v0), float(t0)
    out = {k: [] for k in ("q", "v", "tau", "t")}
    for _ in range(ticks):
        q, v, t, tau = tick(tree, q, v, t, cq, cv, dt_sim, dt_traj, **gains)
        out["q"].append(do.to_f64(q))
        out["v"].append(do.to_f64(v))
        out["tau"].append(do.to_f64(tau))
        out["t"].append(t)
    return {k: np.array(x) for k, x in out.items()}
