"""Shared by tests/test_fit.py (host emulator) and tests/test_gpu_fit.py (GPU):
the fixture tests/golden/fit_cases.npz (make_fit_golden.py), an emulator-backed
stand-in with `ikgrasp.solver.bezier_fit`'s signature, and the comparisons both
suites run.

A case is a path with its parameters; the fixture holds its inputs, the exact
minimiser in 50 digits (double-double, fit_oracle.split), the exact cost, and
the bounds tol_P, tol_curve, tol_cost = 20 x the error of the float64
restatement (fit_oracle.fit_f64: np.linalg.qr of the augmented matrix) against
the 50-digit answer, the factor of the dynamics and rollout fixtures."""
import ctypes as C
import os

import numpy as np

import emu as host_emu
import fit_oracle as fo
from ikgrasp import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 20.0
EPS = 2.0 ** -52

# name -> (n, dim, degree, ridge, T, kind); kind: "smooth" (y_0 = q0), "offset" (y_0 != q0), "zigzag" (cost > 1)
CASES = {
    "n17": (17, 3, 20, 0.0, 1.0, "smooth"),      # the square 15 x 15 interior system: the worst conditioned
    "n18": (18, 3, 20, 0.0, 15.0, "smooth"),
    "n40": (40, 3, 20, 0.0, 1.0, "offset"),
    "n256": (256, 3, 20, 0.0, 15.0, "smooth"),   # the cap
    "n2r": (2, 3, 20, 1e-10, 1.0, "smooth"),
    "n3r": (3, 1, 20, 1e-10, 15.0, "smooth"),
    "n16r": (16, 3, 20, 1e-10, 15.0, "smooth"),
    "n24r": (24, 15, 20, 1e-6, 1.0, "smooth"),
    "d6": (12, 3, 6, 0.0, 1.0, "offset"),        # one free control point
    "d7": (12, 3, 7, 0.0, 15.0, "smooth"),
    "n40w": (40, 15, 20, 0.0, 15.0, "smooth"),   # the robot's width
    "zig": (24, 3, 20, 0.0, 1.0, "zigzag"),      # flag False
}
RAGGED = ("n17", "n2r", "n256", "n40", "n18")    # one call, ridge 1e-10, T = 1
REFERENCE = ("ref0", "ref1", "ref2")             # the reference's own maketraj on small paths


def load():
    return dict(np.load(os.path.join(GOLDEN, "fit_cases.npz")))


def inputs(d, name):
    return d[name + "_q0"], d[name + "_q1"], d[name + "_y"]


def pack(paths):
    return np.concatenate(paths), np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)


class EmuFit:
    """ikg_emu_bezier_fit (libikgrasp_emu.so) behind ikgrasp.solver.bezier_fit's signature, numpy only."""

    def __init__(self):
        self.emu = host_emu.load()

    def bezier_fit(self, q0, q1, path_points, offsets, total_time=1.0, degree=20, ridge=0.0, derivatives=True):
        q0 = np.ascontiguousarray(q0, dtype=np.float64)
        dim = q0.shape[-1]
        q0 = q0.reshape(-1, dim)
        q1 = np.ascontiguousarray(q1, dtype=np.float64).reshape(-1, dim)
        y = np.ascontiguousarray(path_points, dtype=np.float64).reshape(-1, dim)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        B, d = len(q0), int(degree)
        res = {"points": np.full((B, d + 1, dim), -7.0), "cost": np.empty(B), "status": np.empty(B, dtype=np.int32)}
        if derivatives:
            res["vpoints"], res["apoints"] = np.empty((B, d, dim)), np.empty((B, d - 1, dim))
        p = lambda a: None if a is None else a.ctypes.data
        prm = _lib.FitParams(d, float(ridge), float(total_time))
        rc = self.emu.ikg_emu_bezier_fit(p(q0), p(q1), p(y), p(off), B, dim, C.byref(prm),
                                         p(res["points"]), p(res.get("vpoints")), p(res.get("apoints")),
                                         p(res["cost"]), p(res["status"]))
        if rc:
            raise _lib.IkgError(rc, "emulated bezier fit")
        return res


def to_numpy(r):
    return {k: v if isinstance(v, np.ndarray) else v.cpu().numpy() for k, v in r.items()}


def fit_case(fit, d, name):
    n, dim, deg, ridge, T, _ = CASES[name]
    q0, q1, y = inputs(d, name)
    r = to_numpy(fit(q0[None], q1[None], y, np.array([0, n], dtype=np.int64), total_time=T, degree=deg, ridge=ridge))
    assert r["status"][0] == 0
    return {k: v[0] for k, v in r.items()}


def errors(d, name, P, cost):
    """-> (control points / max|P|, curve at 64 parameters / max|curve|, cost / max(cost, sum y^2 2^-52))"""
    deg = CASES[name][2]
    hi, lo = d[name + "_P_hi"], d[name + "_P_lo"]
    dP = fo.diff(P, hi, lo)
    B64 = fo.bernstein(fo.CURVE_U, deg)
    y = d[name + "_y"]
    cost_ref = float(d[name + "_cost"])
    return (np.abs(dP).max() / np.abs(hi).max(), np.abs(B64 @ dP).max() / np.abs(B64 @ hi).max(),
            abs(cost - cost_ref) / max(cost_ref, np.sum(y * y) * EPS))


def check_case(fit, d, name, label):
    """One case against its 50-digit answer under the fixture's bounds; the pinned points bit for bit."""
    n, dim, deg, ridge, T, _ = CASES[name]
    r = fit_case(fit, d, name)
    q0, q1, _ = inputs(d, name)
    P = r["points"]
    for i in range(3):
        assert np.array_equal(P[i], q0) and np.array_equal(P[deg - i], q1), (name, i)
    eP, eC, eJ = errors(d, name, P, r["cost"])
    tP, tC, tJ = (float(d[f"{name}_tol_{k}"]) for k in ("P", "curve", "cost"))
    print(f"{label} {name} (n {n}, dim {dim}, degree {deg}, ridge {ridge:g}, T {T:g}): control points {eP:.2e} "
          f"(bound {tP:.2e}), curve {eC:.2e} (bound {tC:.2e}), cost {r['cost']:.6e}: {eJ:.2e} (bound {tJ:.2e})")
    assert eP <= tP and eC <= tC and eJ <= tJ, (name, eP, tP, eC, tC, eJ, tJ)
    return r


def check_derivatives(r, deg):
    """vpoints / apoints bit-equal to Curve.derivative of the returned points"""
    from ikgrasp.control import Curve
    c = Curve(list(r["points"]), 0.0, 1.0)
    assert np.array_equal(np.array(c.derivative(1).control_points_), r["vpoints"])
    assert np.array_equal(np.array(c.derivative(2).control_points_), r["apoints"])
    assert r["vpoints"].shape[0] == deg and r["apoints"].shape[0] == deg - 1


def ragged_inputs(d):
    q0 = np.array([d[k + "_q0"] for k in RAGGED])
    q1 = np.array([d[k + "_q1"] for k in RAGGED])
    y, off = pack([d[k + "_y"] for k in RAGGED])
    return q0, q1, y, off


def check_ragged(fit, d):
    """Five paths of different lengths in one call equal, bit for bit, the same paths one per call."""
    q0, q1, y, off = ragged_inputs(d)
    kw = dict(total_time=1.0, degree=20, ridge=1e-10)
    batch = to_numpy(fit(q0, q1, y, off, **kw))
    assert np.all(batch["status"] == 0)
    for i in range(len(RAGGED)):
        yi = y[off[i]:off[i + 1]]
        one = to_numpy(fit(q0[i:i + 1], q1[i:i + 1], yi, np.array([0, len(yi)], dtype=np.int64), **kw))
        for k in ("points", "vpoints", "apoints", "cost"):
            assert np.array_equal(batch[k][i], one[k][0]), (RAGGED[i], k)
    return batch


def check_reference(fit, d, name):
    """Against the reference's own maketraj (run at generation time): its
    constraints hold exactly here, our cost is not above its cost, the flag
    agrees.  Control points are NOT compared: SLSQP stops early, and its
    control points differ from the minimiser's by up to 1.5e3 while the costs
    are close."""
    q0, q1, y = inputs(d, name)
    n, T = len(y), float(d[name + "_T"])
    ridge = 0.0 if n >= 17 else 1e-10
    r = to_numpy(fit(q0[None], q1[None], y, np.array([0, n], dtype=np.int64), total_time=T, degree=20, ridge=ridge))
    P, cost = r["points"][0], float(r["cost"][0])
    for i in range(3):
        assert np.array_equal(P[i], q0) and np.array_equal(P[20 - i], q1)
    ref_fun, ref_flag = float(d[name + "_fun"]), bool(d[name + "_flag"])
    print(f"{name}: cost {cost:.3e}, the reference's {ref_fun:.3e}; |P - P_ref| {np.abs(P - d[name + '_P']).max():.2e}")
    assert abs(ref_fun - 0.15) > 0.01
    assert cost <= ref_fun * (1 + 1e-9)
    assert (cost < 0.15) == ref_flag


# ---------------------------------------------------------------- one curve pair per state
def per_state_rollout(solver, q0, v0, sets, t0=None, ticks=0, dt_sim=1e-3, dt_traj=1e-2, record_every=0,
                      outputs=("q", "v", "t"), **gains):
    """IKSolver.rollout(per_state=True), or ikg_emu_control_rollout_curves for rollout_cases.EmuSolver.
    sets = ((points [B,n,nq], t_min, t_max, mult), (vpoints [B,n',nq], t_min, t_max, mult))"""
    if not hasattr(solver, "emu"):
        return solver.rollout(q0, v0, sets, t0=t0, ticks=ticks, dt_sim=dt_sim, dt_traj=dt_traj,
                              record_every=record_every, outputs=outputs, per_state=True, **gains)
    nq = solver.nq
    keep = [np.ascontiguousarray(s[0], dtype=np.float64) for s in sets]
    bs = [_lib.BezierSet(k.ctypes.data, k.shape[1], float(s[1]), float(s[2]), float(s[3])) for k, s in zip(keep, sets)]
    prm = _lib.rollout_params(ticks, dt_sim, dt_traj, record_every, **gains)
    q0 = np.ascontiguousarray(q0, dtype=np.float64).reshape(-1, nq)
    v0 = None if v0 is None else np.ascontiguousarray(v0, dtype=np.float64).reshape(-1, nq)
    t0 = None if t0 is None else np.ascontiguousarray(t0, dtype=np.float64).reshape(-1)
    B = len(q0)
    R = ticks // record_every if record_every else 0
    shape = lambda k: (B,) if k == "t" else ((B, R, nq) if k.endswith("_hist") else (B, nq))
    res = {k: np.empty(shape(k)) for k in outputs}
    out = _lib.RolloutOut(*[None if k not in res else res[k].ctypes.data
                            for k in ("q", "v", "t", "q_hist", "v_hist", "tau_hist")])
    p = lambda a: None if a is None else a.ctypes.data
    rc = solver.emu.ikg_emu_control_rollout_curves(C.byref(solver.desc), C.byref(solver.idesc), p(q0), p(v0), p(t0), B,
                                                   C.byref(bs[0]), C.byref(bs[1]), C.byref(prm), C.byref(out))
    if rc:
        raise _lib.IkgError(rc, "emulated per-state rollout")
    return res


HIST = ("q_hist", "v_hist", "tau_hist")


def tile(curve, B, like=None):
    """a shared curve (points, t_min, t_max, mult) as B equal per-state curves"""
    pts = np.ascontiguousarray(np.broadcast_to(np.asarray(curve[0], dtype=np.float64), (B,) + np.shape(curve[0])))
    return (pts if like is None else like(pts),) + tuple(curve[1:])


def check_equal_curves_match_shared(solver, rd, ticks=8, like=None, back=np.asarray):
    """B equal curves: the per-state entry equals the shared-curve entry bit for
    bit, on the rollout fixture's 16 starts (every group of curves and gains)."""
    import rollout_cases as rc
    seen = 0
    for rows, (cq, cv), gains in rc.groups(rd, "nextage"):
        if len(rows) == 0:
            continue
        q0, v0, t0 = rd["ro_q0"][rows], rd["ro_v0"][rows], rd["ro_t0"][rows]
        conv = (lambda x: x) if like is None else like
        kw = dict(t0=conv(t0), ticks=ticks, record_every=1, outputs=HIST + ("q", "v", "t"), **gains)
        shared = solver.rollout(conv(q0), conv(v0), (cq, cv), **kw)
        mine = per_state_rollout(solver, conv(q0), conv(v0), (tile(cq, len(rows), like), tile(cv, len(rows), like)), **kw)
        for k in shared:
            assert np.array_equal(back(shared[k]), back(mine[k])), (k, rows)
        seen += len(rows)
    assert seen == 16


def distinct_curves(rd):
    """4 curve pairs of one size from the rollout fixture's first trajectory: itself, run backwards, the mean of
    the two and a scaled copy -> (Pq [4,n,nq], Pv [4,n-1,nq], t_min, t_max)"""
    import rollout_cases as rc
    import rollout_oracle as ro
    (P1, t_min, t_max, _), _ = rc.traj_curves(rd, 1, False)
    P2 = P1[::-1].copy()
    Pq = np.array([P1, P2, 0.5 * (P1 + P2), 0.9 * P1])
    Pv = np.array([ro.derivative((P, t_min, t_max, 1.0))[0] for P in Pq])
    return Pq, Pv, float(t_min), float(t_max)


def check_distinct_curves_match_single(solver, rd, ticks=8, like=None, back=np.asarray):
    """4 distinct curves: state p equals, bit for bit, a B = 1 shared-curve rollout on curve p."""
    Pq, Pv, t_min, t_max = distinct_curves(rd)
    mv = 1.0 * (1.0 / (t_max - t_min))
    conv = (lambda x: x) if like is None else like
    q0, v0, t0 = rd["ro_q0"][:4], rd["ro_v0"][:4], rd["ro_t0"][:4]
    kw = dict(ticks=ticks, record_every=1, outputs=HIST + ("q", "v", "t"), fc_bias=np.zeros(12))
    mine = per_state_rollout(solver, conv(q0), conv(v0), ((conv(Pq), t_min, t_max, 1.0), (conv(Pv), t_min, t_max, mv)),
                             t0=conv(t0), **kw)
    for p in range(4):
        one = solver.rollout(conv(q0[p:p + 1]), conv(v0[p:p + 1]), ((Pq[p], t_min, t_max, 1.0), (Pv[p], t_min, t_max, mv)),
                             t0=conv(t0[p:p + 1]), **kw)
        for k in one:
            assert np.array_equal(back(one[k])[0], back(mine[k])[p]), (k, p)
    assert not np.array_equal(back(mine["q_hist"])[0], back(mine["q_hist"])[1])


# ---------------------------------------------------------------- fit, then track
def tracking_paths(rd):
    """4 paths of the robot's width: the rollout fixture's first trajectory sampled at 17, 24, 40 and 64 times
    (float64 Horner) with seeded noise of 1e-5 rad on the interior points -> (q0s, q1s, paths, T).
    The exact fit amplifies sample noise into the control polygon (8e5 x at n = 17), and Horner's rounding error
    grows with max|P|: the noise keeps the fitted polygons (max|P| about 12) inside the range of the rollout
    fixture's own curves (max|P| = 88), on which its per-tick bounds were measured."""
    import rollout_cases as rc
    (P1, t_min, t_max, _), _ = rc.traj_curves(rd, 1, False)
    T = float(t_max - t_min)
    rng = np.random.default_rng(11)
    paths = []
    for n in (17, 24, 40, 64):
        t, _ = fo.times(n, T)
        y = np.array([fo.horner(P1, tk, T) for tk in t])
        y[1:-1] += 1e-5 * rng.standard_normal((n - 2, y.shape[1]))
        paths.append(y)
    B = len(paths)
    return np.tile(P1[0], (B, 1)), np.tile(P1[-1], (B, 1)), paths, T


def check_fit_then_track(fit, solver, rd, label, ticks=16, like=None, back=np.asarray):
    """End to end: fit 4 paths, follow each with its own loop for `ticks` ticks
    (fc_bias = 0, from the rollout fixture's first four starts: states and
    clocks its bounds were measured on, a few hundredths of a radian off the
    curve.  A start exactly on the curve at rest makes the rotation error a
    rounding-sized angle, where the oracle's and the kernel's log3 differ by
    more than these bounds), and compare with
    the numpy rollout oracle (tests/rollout_oracle.py, float64) fed the SAME
    fitted control points, under the rollout fixture's per-tick bounds as that
    fixture applies them (rollout_cases.check_rollouts): tol_q, tol_v, tol_tau
    times the maximum of the FIXTURE's reference output, the same absolute
    bounds the same starts meet there.  (These 16 ticks without the contact
    bias move less than the fixture's 32 with it; bounds relative to this
    run's own maxima would be tighter than the ones measured.)"""
    import dynamics_oracle as do
    import rollout_cases as rc
    import rollout_oracle as ro
    q0s, q1s, paths, T = tracking_paths(rd)
    y, off = pack(paths)
    r = to_numpy(fit(q0s, q1s, y, off, total_time=T, degree=20, ridge=0.0))
    assert np.all(r["status"] == 0) and np.all(r["cost"] < 0.15)
    assert np.abs(r["points"]).max() < 88.0
    P, V = r["points"], r["vpoints"]
    mv = 1.0 * (1.0 / T)
    conv = (lambda x: x) if like is None else like
    x0, v0, t0 = rd["ro_q0"][:4], rd["ro_v0"][:4], rd["ro_t0"][:4]
    got = per_state_rollout(solver, conv(x0), conv(v0), ((conv(P), 0.0, T, 1.0), (conv(V), 0.0, T, mv)), t0=conv(t0),
                            ticks=ticks, record_every=1, outputs=HIST, fc_bias=np.zeros(12))
    m, bi = rc.models()["nextage"]
    tree = do.Tree(do.F64, m, bi)
    tol = rc.tolerances(rd, "nextage")
    want = [ro.rollout(tree, x0[p], v0[p], float(t0[p]), (P[p], 0.0, T, 1.0), (V[p], 0.0, T, mv), ticks, fc_bias=np.zeros(12))
            for p in range(len(paths))]
    for k in rc.OUT:
        ref = np.array([w[k] for w in want])
        scale = np.abs(rd[f"ro_{k}_mp"]).max()
        err = np.abs(back(got[k + "_hist"]) - ref).max(axis=(0, 2)) / scale
        j = int(np.argmax(err / tol[k][:ticks]))
        print(f"{label} fit-then-track {k}: largest {err.max():.3e} of the fixture's max|{k}| = {scale:.3g} (this run's "
              f"{np.abs(ref).max():.3g}); closest to its bound at tick {j}: {err[j]:.3e} (bound {tol[k][j]:.3e})")
        assert np.all(err <= tol[k][:ticks]), (k, j, err[j], tol[k][j])
