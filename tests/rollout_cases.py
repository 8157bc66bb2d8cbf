"""Shared by tests/test_rollout.py (host emulator) and tests/test_gpu_rollout.py
(GPU): the fixture tests/golden/rollout_cases.npz (make_rollout_golden.py), the
models it was made for, an emulator-backed stand-in with IKSolver's methods,
and the comparisons both suites run."""
import ctypes as C
import os

import numpy as np

import dynamics_oracle as do
import emu as host_emu
from ikgrasp import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
OUT = ("q", "v", "tau")


def load():
    return dict(np.load(os.path.join(GOLDEN, "rollout_cases.npz")))


def models():
    """name -> (DualArmModel, BodyInertias), as make_rollout_golden.load_model"""
    import robot_family
    from ikgrasp.model import DualArmModel, load_nextage, load_nextage_inertia
    tilted = DualArmModel.from_urdf(os.path.join(GOLDEN, "tilted_dualarm.urdf"), os.path.join(GOLDEN, "tilted_cube.urdf"))
    mixed = robot_family.load_model("mixed_axes")
    return {"nextage": (load_nextage(), load_nextage_inertia()), "tilted": (tilted, do.seeded_inertias(tilted.nq, 1)),
            "mixed": (mixed, do.seeded_inertias(mixed.nq, 3))}


def gains_alt():
    dc = np.load(os.path.join(GOLDEN, "dynamics_cases.npz"))
    g = dict(zip(("Kp", "Kv", "Kf", "Kt", "lambda_reg", "qp_reg"), (float(x) for x in dc["gains_alt"])))
    g["fc_bias"] = np.zeros(12)
    return g


def traj_curves(d, i, vfile):
    t_min, t_max, mult = d[f"traj{i}_range"]
    cq = (d[f"traj{i}_q"], t_min, t_max, mult)
    cv = (d[f"traj{i}_vfile"], t_min, t_max, mult) if vfile else (d[f"traj{i}_vder"], t_min, t_max,
                                                                  mult * (1.0 / (t_max - t_min)))
    return cq, cv


def groups(d, name):
    """The fixture's rollouts of one model as calls: [(rows, (cq, cv), gains)]"""
    alt = gains_alt()
    if name == "nextage":
        out = []
        for tr in (1, 2):
            for vfile in (False, True):
                for use_alt in (False, True):
                    rows = np.flatnonzero((d["ro_traj"] == tr) & (d["ro_vfile"] == vfile) & (d["ro_alt"] == use_alt))
                    out.append((rows, traj_curves(d, tr, vfile), alt if use_alt else {}))
        return out
    t_min, t_max, mq, mv = d[f"{name}_range"]
    cv = ((d[f"{name}_cq"], t_min, t_max, mq), (d[f"{name}_cv"], t_min, t_max, mv))
    return [(np.flatnonzero(d[f"{name}_alt"] == a), cv, alt if a else {}) for a in (False, True)]


def prefix(name):
    return "ro_" if name == "nextage" else name + "_"


def tolerances(d, name):
    return {k: d["tol_" + k] if name == "nextage" else d[f"{name}_tol_{k}"] for k in OUT}


# ---------------------------------------------------------------- the emulator behind IKSolver's methods
class EmuSolver:
    """ikg_emu_* (libikgrasp_emu.so, tests/emu.py) with the signatures of IKSolver.rollout /
    forward_dynamics / bezier / control_torques, numpy only."""

    def __init__(self, model, inertias):
        self.emu, self.model, self.inertias, self.nq = host_emu.load(), model, inertias, model.nq
        self.desc = _lib.model_desc(model)
        self.idesc = _lib.inertia_desc(inertias) if inertias is not None else None

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def _rows(self, x, w=None):
        return None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1, w or self.nq)

    def dynamics(self, q, v=None, outputs=("M", "nle")):
        return host_emu.dynamics(self.model, self.inertias, q, v, outputs=("M", "nle"))

    def forward_dynamics(self, q, v, tau):
        q, v, tau = self._rows(q), self._rows(v), self._rows(tau)
        out = np.empty_like(q)
        rc = self.emu.ikg_emu_forward_dynamics(C.byref(self.desc), C.byref(self.idesc), self._p(q), self._p(v),
                                               self._p(tau), len(q), self._p(out))
        if rc:
            raise _lib.IkgError(rc, "emulated forward dynamics")
        return out

    def bezier(self, points, t_min, t_max, mult, times):
        pts, t_min, t_max, mult = _lib.curve((points, t_min, t_max, mult))
        tt = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        out = np.empty((len(tt), pts.shape[1]))
        rc = self.emu.ikg_emu_bezier(self._p(pts), pts.shape[0], pts.shape[1], float(t_min), float(t_max), float(mult),
                                     self._p(tt), len(tt), self._p(out))
        if rc:
            raise _lib.IkgError(rc, "emulated bezier")
        return out

    def control_torques(self, q, v, q_des, v_des, outputs=("tau",), **gains):
        q, v, qd, vd = (self._rows(x) for x in (q, v, q_des, v_des))
        B, nq = q.shape
        J, dJv, e, ed = np.empty((B, 12, nq)), np.empty((B, 12)), np.empty((B, 12)), np.empty((B, 12))
        assert self.emu.ikg_emu_frame_terms(C.byref(self.desc), self._p(q), self._p(v), self._p(qd), self._p(vd),
                                            B, self._p(J), self._p(dJv), self._p(e), self._p(ed)) == 0
        return host_emu.control_torque(self.model, self.inertias, q, v, J, dJv, e, ed, outputs=("tau",), **gains)

    def rollout(self, q0, v0, trajs, t0=None, ticks=0, dt_sim=1e-3, dt_traj=1e-2, record_every=0,
                outputs=("q", "v", "t"), **gains):
        nq = self.nq
        bq, keep_q = _lib.bezier_desc(trajs[0], nq)
        bv, keep_v = _lib.bezier_desc(trajs[1], nq)
        prm = _lib.rollout_params(ticks, dt_sim, dt_traj, record_every, **gains)
        q0, v0 = self._rows(q0), self._rows(v0)
        t0 = None if t0 is None else np.ascontiguousarray(t0, dtype=np.float64).reshape(-1)
        B = len(q0)
        R = ticks // record_every if record_every else 0
        shape = lambda k: (B,) if k == "t" else ((B, R, nq) if k.endswith("_hist") else (B, nq))
        res = {k: np.empty(shape(k)) for k in outputs}
        out = _lib.RolloutOut(*[None if k not in res else res[k].ctypes.data
                                for k in ("q", "v", "t", "q_hist", "v_hist", "tau_hist")])
        rc = self.emu.ikg_emu_control_rollout(C.byref(self.desc), C.byref(self.idesc), self._p(q0), self._p(v0),
                                              self._p(t0), B, C.byref(bq), C.byref(bv), C.byref(prm), C.byref(out))
        if rc:
            raise _lib.IkgError(rc, "emulated rollout")
        return res


# ---------------------------------------------------------------- comparisons
HIST = ("q_hist", "v_hist", "tau_hist")


def bezier_bound(points, mult):
    """4 n 2^-52 max|P| |mult|: the Bernstein weights are a partition of unity,
    so Horner's rounding (n steps of a few operations on values bounded by
    max|P|) stays below it."""
    P = np.asarray(points)
    return 4 * len(P) * EPS * np.abs(P).max() * abs(mult)


def check_bezier(solver, d):
    worst = 0.0
    for i in (1, 2):
        for k, vfile in (("q", None), ("vder", False), ("vfile", True)):
            cq, cv = traj_curves(d, i, bool(vfile))
            pts, t_min, t_max, mult = cq if k == "q" else cv
            got = solver.bezier(pts, t_min, t_max, mult, d["bez_times"])
            got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
            err = np.abs(got - d[f"bez_traj{i}_{k}_mp"]).max()
            bound = bezier_bound(pts, mult)
            print(f"bezier traj{i}_{k}: |d| {err:.2e} (bound {bound:.2e}; float64 restatement "
                  f"{np.abs(d[f'bez_traj{i}_{k}_f64err']).max():.2e})")
            assert err <= bound, (i, k)
            worst = max(worst, err / bound)
    return worst


def check_forward_dynamics(solver, q, v, tau, ref, tol, label):
    qdd = solver.forward_dynamics(q, v, tau)
    err = np.abs(qdd - ref).max() / np.abs(ref).max()
    print(f"{label} forward dynamics: {err:.3e} of max|qdd| (bound {tol:.3e})")
    assert err <= tol
    return qdd


def check_forward_dynamics_equation(solver, q, v, tau, tol, label):
    """M qdd + nle == tau with the solver's own M and nle.  The bound is the
    fixture's, relative to max (|M| |qdd|): M qdd cancels against nle - tau
    (|M| |qdd| is up to 1e3 x |tau| on the near-singular states), and a
    backward-stable solve leaves a residual proportional to |M| |qdd|, not |tau|."""
    qdd = solver.forward_dynamics(q, v, tau)
    dyn = solver.dynamics(q, v, outputs=("M", "nle"))
    res = np.einsum("bij,bj->bi", dyn["M"], qdd) + dyn["nle"] - tau
    scale = np.einsum("bij,bj->bi", np.abs(dyn["M"]), np.abs(qdd)).max()
    print(f"{label} |M qdd + nle - tau| {np.abs(res).max():.3e} = {np.abs(res).max() / scale:.3e} of max |M||qdd| "
          f"(bound {tol:.3e})")
    assert np.abs(res).max() <= tol * scale


def run_rollouts(solver, d, name, ticks, **kw):
    """The fixture's starts of one model through solver.rollout -> {q, v, tau: [n, ticks, nq]}"""
    pre = prefix(name)
    n = len(d[pre + "q0"])
    got = {k: np.empty((n, ticks, solver.nq)) for k in OUT}
    for rows, trajs, gains in groups(d, name):
        r = solver.rollout(d[pre + "q0"][rows], d[pre + "v0"][rows], trajs, t0=d[pre + "t0"][rows], ticks=ticks,
                           record_every=1, outputs=HIST, **gains, **kw)
        for k in OUT:
            got[k][rows] = r[k + "_hist"]
    return got


def check_rollouts(got, d, name, label):
    """Every tick within the per-tick bound; returns the largest error / bound per output."""
    pre, tol, worst = prefix(name), tolerances(d, name), {}
    for k in OUT:
        ref = d[f"{pre}{k}_mp"]
        ticks = ref.shape[1]
        err = np.abs(got[k] - ref).max(axis=(0, 2)) / np.abs(ref).max()
        j = int(np.argmax(err / tol[k]))
        worst[k] = float(err.max())
        print(f"{label} {name} {k}: largest error {err.max():.3e} of max|.|; closest to its bound at tick {j}: "
              f"{err[j]:.3e} (bound {tol[k][j]:.3e}); last tick {err[-1]:.3e} (bound {tol[k][ticks - 1]:.3e})")
        assert np.all(err <= tol[k]), (name, k, j, err[j], tol[k][j])
    return worst
