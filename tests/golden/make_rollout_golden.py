"""Writes tests/golden/rollout_cases.npz from tests/rollout_oracle.py.

    python tests/golden/make_rollout_golden.py

Reads the reference's trajectory.json / trajectory2.json (data only: the
control points) and tests/golden/dynamics_cases.npz.  Every quantity X is
stored as X_mp (the 50-digit evaluation rounded to float64: the truth) and
X_f64err (float32: the float64 restatement minus X_mp; the restatement itself
is X_mp + X_f64err to float32 accuracy of the difference).

Entries
  traj{1,2}_q, _vder, _vfile   control points [n,15] of the q curve, of its derivative as
                               Bezier.derivative(1) builds it (degree dP, mult 1/T) and of the
                               velocity curve as the file stores it (loaded with the file's mult_t)
  traj{1,2}_range              t_min, t_max, mult_t of the file
  bez_times [64], bez_{curve}_mp / _f64err [64,15]   curve values at t_min, t_max, 30 accumulated
                               multiples of 0.01 and seeded times, for the six curves above
  fd_qdd_mp / _f64err [96,15]  forward dynamics of the states of dynamics_cases.npz with their tau
  tol_fd                       20 x the float64 error relative to max|qdd| (make_dynamics_golden.py's convention)
  ro_q0, ro_v0 [16,15], ro_t0 [16], ro_traj, ro_vfile, ro_alt [16]   the starts: trajectory 1/2, the
                               file-loaded v curve or the derivative, the alternative gains (fc_bias = 0) or the defaults
  ro_{q,v,tau}_mp / _f64err [16,32,15]   every tick recorded
  tol_q, tol_v, tol_tau [32]   per tick: 20 x the running maximum, over ticks <= k and all cases, of the
                               float64 restatement's error against 50 digits, relative to max|output_mp|
  tilted_* / mixed_*           the same for tests/golden/tilted_dualarm.urdf (4 starts x 16 ticks) and the
                               family's mixed_axes.urdf (nq = 32; 2 starts x 8 ticks, 16 forward-dynamics
                               states) with seeded inertias and seeded control points
The printed envelopes are quoted in DESIGN.md §2d.2.
"""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "motion-planning-and-control-for-dual-manipulator-robot_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dynamics_oracle as do  # noqa: E402
import rollout_oracle as ro  # noqa: E402

REFERENCE = "/root/reference"
T0 = (0.0, 3.0, 7.5, 14.8)
TICKS = 32
SEEDS = {"tilted": 1, "mixed": 3}  # dynamics_oracle.seeded_inertias


def load_model(name):
    from ikgrasp.model import DualArmModel, load_nextage, load_nextage_inertia
    if name == "nextage":
        return load_nextage(), load_nextage_inertia()
    if name == "tilted":
        m = DualArmModel.from_urdf(os.path.join(HERE, "tilted_dualarm.urdf"), os.path.join(HERE, "tilted_cube.urdf"))
    else:
        import robot_family
        m = robot_family.load_model("mixed_axes")
    return m, do.seeded_inertias(m.nq, SEEDS[name])


def gains_alt():
    dc = np.load(os.path.join(HERE, "dynamics_cases.npz"))
    g = dict(zip(("Kp", "Kv", "Kf", "Kt", "lambda_reg", "qp_reg"), (float(x) for x in dc["gains_alt"])))
    g["fc_bias"] = np.zeros(12)
    return g


def seeded_curve(model, n_points, t_max, seed):
    """A smooth seeded q curve inside the joint limits and its derivative."""
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(model.lower, -1.5), np.minimum(model.upper, 1.5)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    P = mid + 0.5 * half * np.cumsum(rng.uniform(-0.25, 0.25, (n_points, model.nq)), axis=0)
    cq = (P, 0.0, t_max, 1.0)
    return cq, ro.derivative(cq)


def _rollout(args):
    name, q0, v0, t0, cq, cv, ticks, gains = args
    model, inert = load_model(name)
    out = {}
    for tag, ar in (("f64", do.F64), ("mp", do.MP)):
        r = ro.rollout(do.Tree(ar, model, inert), q0, v0, t0, cq, cv, ticks, **gains)
        out.update({f"{k}_{tag}": r[k] for k in ("q", "v", "tau")})
    return out


def _fd(args):
    name, q, v, tau = args
    model, inert = load_model(name)
    return (do.to_f64(ro.forward_dynamics(do.Tree(do.F64, model, inert), q, v, tau)),
            do.to_f64(ro.forward_dynamics(do.Tree(do.MP, model, inert), q, v, tau)))


def _bezier(args):
    curve, times = args
    return (np.array([do.to_f64(ro.bezier(do.F64, curve, t)) for t in times]),
            np.array([do.to_f64(ro.bezier(do.MP, curve, t)) for t in times]))


def store(d, key, f64, mp):
    d[key + "_mp"] = mp
    d[key + "_f64err"] = (f64 - mp).astype(np.float32)


def starts(cq, cv, t0, rng):
    """desired state at t0 plus a seeded error (sigma 0.02 on q, 0.05 on v)"""
    qd = ro.bezier(do.F64, cq, ro.clamp(cq, t0))
    vd = ro.bezier(do.F64, cv, ro.clamp(cv, t0))
    return qd + rng.normal(0.0, 0.02, qd.shape), vd + rng.normal(0.0, 0.05, vd.shape)


def envelopes(d, pre, res, ticks, label):
    """per-tick bounds from the float64 restatement's error against 50 digits"""
    for k in ("q", "v", "tau"):
        f64 = np.array([r[k + "_f64"] for r in res])
        mp = np.array([r[k + "_mp"] for r in res])
        store(d, f"{pre}{k}", f64, mp)
        env = np.maximum.accumulate(np.abs(f64 - mp).max(axis=(0, 2))) / np.abs(mp).max()
        d[f"{pre}tol_{k}"] = 20.0 * env
        print(f"{label} {k:3s}: float64 vs 50 digits relative to max|.| = {np.abs(mp).max():.3g}: tick 0 {env[0]:.2e}, "
              f"tick {ticks // 2 - 1} {env[ticks // 2 - 1]:.2e}, tick {ticks - 1} {env[-1]:.2e} (bounds = 20 x)")


def main():
    d = {}
    pool = Pool(min(16, os.cpu_count() or 1))
    # ---- the reference's two trajectories
    curves = {}
    for i, fn in ((1, "trajectory.json"), (2, "trajectory2.json")):
        with open(os.path.join(REFERENCE, fn)) as f:
            tj = json.load(f)
        rng_ = (float(tj["t_min"]), float(tj["t_max"]), float(tj["mult_t"]))
        cq = (np.array(tj["q_control_points"], dtype=np.float64),) + rng_
        cvder = ro.derivative(cq)
        cvfile = (np.array(tj["vq_control_points"], dtype=np.float64),) + rng_
        d[f"traj{i}_q"], d[f"traj{i}_vder"], d[f"traj{i}_vfile"] = cq[0], cvder[0], cvfile[0]
        d[f"traj{i}_range"] = np.array(rng_)
        curves[i] = {"q": cq, "vder": cvder, "vfile": cvfile}
    # ---- Bezier samples
    t_min, t_max = curves[1]["q"][1], curves[1]["q"][2]
    acc, t = [], t_min
    for _ in range(30):
        t += 0.01
        acc.append(t)
    rng = np.random.default_rng(2025)
    times = np.array([t_min, t_max] + acc + list(rng.uniform(t_min, t_max, 32)))
    d["bez_times"] = times
    names = [(i, k) for i in (1, 2) for k in ("q", "vder", "vfile")]
    for (i, k), (f64, mp) in zip(names, pool.map(_bezier, [(curves[i][k], times) for i, k in names])):
        store(d, f"bez_traj{i}_{k}", f64, mp)
        print(f"bezier traj{i}_{k}: float64 vs 50 digits {np.abs(f64 - mp).max():.2e} (max|.| {np.abs(mp).max():.3g})")
    # ---- forward dynamics of the dynamics_cases states
    dc = np.load(os.path.join(HERE, "dynamics_cases.npz"))
    res = pool.map(_fd, [("nextage", dc["q"][i], dc["v"][i], dc["tau"][i]) for i in range(len(dc["q"]))])
    f64, mp = np.array([r[0] for r in res]), np.array([r[1] for r in res])
    store(d, "fd_qdd", f64, mp)
    d["tol_fd"] = 20.0 * np.abs(f64 - mp).max() / np.abs(mp).max()
    print(f"forward dynamics: float64 vs 50 digits {np.abs(f64 - mp).max() / np.abs(mp).max():.2e} of max|qdd| = "
          f"{np.abs(mp).max():.3g} (bound {float(d['tol_fd']):.2e})")
    # ---- rollouts on the reference's trajectories
    alt = gains_alt()
    rng = np.random.default_rng(31)
    jobs, meta = [], []
    for i in range(16):
        t0, tr, vfile, use_alt = T0[i % 4], 1 + (i // 4) % 2, i >= 8, i % 2 == 1
        cq, cv = curves[tr]["q"], curves[tr]["vfile" if vfile else "vder"]
        q0, v0 = starts(cq, cv, t0, rng)
        jobs.append(("nextage", q0, v0, t0, cq, cv, TICKS, alt if use_alt else {}))
        meta.append((q0, v0, t0, tr, vfile, use_alt))
    res = pool.map(_rollout, jobs)
    d["ro_q0"], d["ro_v0"] = np.array([m[0] for m in meta]), np.array([m[1] for m in meta])
    d["ro_t0"] = np.array([m[2] for m in meta])
    d["ro_traj"] = np.array([m[3] for m in meta], dtype=np.int32)
    d["ro_vfile"] = np.array([m[4] for m in meta])
    d["ro_alt"] = np.array([m[5] for m in meta])
    envelopes(d, "ro_", res, TICKS, "nextage")
    for k in ("q", "v", "tau"):  # the issue's names
        d["tol_" + k] = d.pop(f"ro_tol_{k}")
    # ---- the other models: seeded inertias and control points
    for name, n_starts, ticks, n_points, t_end, n_fd in (("tilted", 4, 16, 6, 2.0, 0), ("mixed", 2, 8, 5, 1.0, 16)):
        model, _ = load_model(name)
        cq, cv = seeded_curve(model, n_points, t_end, 100 + SEEDS[name])
        d[f"{name}_cq"], d[f"{name}_cv"] = cq[0], cv[0]
        d[f"{name}_range"] = np.array([cq[1], cq[2], cq[3], cv[3]])
        rng = np.random.default_rng(200 + SEEDS[name])
        t0s = [t_end * x for x in (0.0, 0.25, 0.5, 0.95)][:n_starts] if n_starts > 2 else [0.0, 0.95 * t_end]
        jobs, q0s, v0s = [], [], []
        for i, t0 in enumerate(t0s):
            q0, v0 = starts(cq, cv, t0, rng)
            q0s.append(q0)
            v0s.append(v0)
            jobs.append((name, q0, v0, t0, cq, cv, ticks, alt if i % 2 else {}))
        res = pool.map(_rollout, jobs)
        d[f"{name}_q0"], d[f"{name}_v0"], d[f"{name}_t0"] = np.array(q0s), np.array(v0s), np.array(t0s)
        d[f"{name}_alt"] = np.array([i % 2 == 1 for i in range(n_starts)])
        envelopes(d, f"{name}_", res, ticks, name)
        if n_fd:
            q = rng.uniform(np.maximum(model.lower, -1.5), np.minimum(model.upper, 1.5), (n_fd, model.nq))
            v, tau = rng.normal(0.0, 0.5, (n_fd, model.nq)), rng.normal(0.0, 20.0, (n_fd, model.nq))
            res = pool.map(_fd, [(name, q[i], v[i], tau[i]) for i in range(n_fd)])
            f64, mp = np.array([r[0] for r in res]), np.array([r[1] for r in res])
            d[f"{name}_fd_q"], d[f"{name}_fd_v"], d[f"{name}_fd_tau"] = q, v, tau
            store(d, f"{name}_fd_qdd", f64, mp)
            d[f"{name}_tol_fd"] = 20.0 * np.abs(f64 - mp).max() / np.abs(mp).max()
            print(f"{name} forward dynamics: float64 vs 50 digits {np.abs(f64 - mp).max() / np.abs(mp).max():.2e} "
                  f"of max|qdd| (bound {float(d[name + '_tol_fd']):.2e})")
    pool.close()
    path = os.path.join(HERE, "rollout_cases.npz")
    np.savez_compressed(path, **d)
    print(f"wrote rollout_cases.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
