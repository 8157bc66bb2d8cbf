"""Trajectory-dynamics benchmark (fp64): ikg_trajectory_dynamics_batch against
the composed route through the entry points that existed before it.

Curves: B seeded noisy copies of the reference's recorded trajectory
(tests/golden/rollout_cases.npz `traj1_q`, 16 control points, nq = 15), S = 151
samples each, the URDF's velocity and effort limits, T = 15 s.

  fused             one call of ikg_trajectory_dynamics_batch with device
                    pointers, the per-curve reductions only
  fused+samples     the same with tau and g per sample
  composed_resident ikg_dynamics_batch (M, nle, g) on the B S states already on
                    the device, then tau = M a + nle in torch: the composed
                    route without its curve evaluation, its lower bound
  composed          per curve three calls of ikg_bezier_eval_batch (q, v, a),
                    then composed_resident and the ratios folded in numpy (at
                    most --composed-max curves: 3 B host calls)

All are timed in one process, alternated `--reps` times after a warm-up of
every shape, with the host clock around windows of back-to-back calls that end
in a device synchronise, each window at least `--window` seconds of work.
Reported per route: median and (min, max) seconds per call, the bytes each
route must move to and from device memory (from the shapes) and the rate they
give over the median, and the two routes' largest difference in tau and g.

    python tools/bench_trajdyn.py [--batches 256,4096] [--samples 151] [--reps 5] [--window 0.3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "motion-planning-and-control-for-dual-manipulator-robot_amd")):
    sys.path.insert(0, p)

PARTIAL_BYTES = 72  # TrajDynPartial: four (value, sample, joint) and a count


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "runs": len(xs)}


def launcher_chunks(B, S, side=4):
    """runs per curve at samples_per_wave = 0 (trajdyn_samples_per_wave, csrc/ikg_dynamics.hpp; nq <= 16)"""
    want = -(-8192 // B)
    spw = -(-(-(-S // want)) // side) * side
    spw = min(max(spw, 1), S)
    return -(-S // spw)


def sample_times(t_max, S):
    t = np.array([(k * t_max) / (S - 1) for k in range(S)])
    t[-1] = t_max
    return t


def curve_states(solver, pts, t_max, S):
    """q, v, a [B S, nq] of the curves, three ikg_bezier_eval_batch calls per curve"""
    from ikgrasp.control import Curve
    times = sample_times(t_max, S)
    rows = [[], [], []]
    for P in pts:
        c = Curve(list(P), 0.0, t_max)
        for i, x in enumerate((c, c.derivative(1), c.derivative(2))):
            rows[i].append(solver.bezier(np.array(x.control_points_), x.T_min_, x.T_max_, x.mult_T_, times))
    return tuple(np.concatenate(r) for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--samples", type=int, default=151)
    ap.add_argument("--noise", type=float, default=0.05, help="rad of seeded noise on the inner control points")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window, at least")
    ap.add_argument("--composed-max", type=int, default=256, help="largest batch the full composed route is timed at")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_trajdyn.py needs a ROCm GPU: a time taken elsewhere says nothing about the kernels")
    import ikgrasp
    robot = ikgrasp.setuppinocchio()[0]
    s, act = robot.solver, robot.actuation
    P = np.load(os.path.join(ROOT, "tests", "golden", "rollout_cases.npz"))["traj1_q"]
    n, nq, S, T = len(P), P.shape[1], a.samples, 15.0
    lines = []
    for B in [int(x) for x in a.batches.split(",")]:
        rng = np.random.default_rng(B)
        pts = P[None] + a.noise * rng.standard_normal((B,) + P.shape)
        pts[:, 0], pts[:, -1] = P[0], P[-1]
        pts = np.ascontiguousarray(pts)
        dpts = torch.as_tensor(pts, device="cuda")
        q, v, acc = curve_states(s, pts[:min(B, a.composed_max)], T, S)
        reps = -(-B // min(B, a.composed_max))  # the resident route's states: the evaluated curves, tiled to B S rows
        dq, dv, da = (torch.as_tensor(np.tile(x, (reps, 1))[:B * S], device="cuda") for x in (q, v, acc))

        def resident():
            r = s.dynamics(dq, dv, outputs=("M", "nle", "g"))
            return torch.einsum("kij,kj->ki", r["M"], da) + r["nle"], r["g"]

        def composed():
            b = min(B, a.composed_max)
            cq, cv, ca = curve_states(s, pts[:b], T, S)
            r = s.dynamics(cq, cv, outputs=("M", "nle", "g"))
            tau = (np.einsum("kij,kj->ki", r["M"], ca) + r["nle"]).reshape(b, S, nq)
            g = r["g"].reshape(b, S, nq)
            return {"tau": tau, "g": g, "speed_scale": (np.abs(cv).reshape(b, S, nq) / act.velocity).max(axis=(1, 2)),
                    "torque_use": (np.abs(tau) / act.effort).max(axis=(1, 2)),
                    "static_use": (np.abs(g) / act.effort).max(axis=(1, 2))}

        kw = dict(samples=S, velocity=act.velocity, effort=act.effort)
        routes = {"fused": lambda: s.curve_dynamics(dpts, 0.0, T, **kw),
                  "fused+samples": lambda: s.curve_dynamics(dpts, 0.0, T, per_sample=True, **kw),
                  "composed_resident": resident, "composed": composed}
        last, calls = {}, {}
        for k, run in routes.items():  # warm-up of every shape; its second call sizes the window
            run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = run()
            torch.cuda.synchronize()
            calls[k] = max(1, int(np.ceil(a.window / (time.perf_counter() - t0))))
        t = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, run in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls[k]):
                    last[k] = run()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / calls[k])
        f = {k: x.cpu().numpy() for k, x in last["fused+samples"].items()}
        g = last["composed"]
        b = len(g["tau"])
        N = B * S
        chunks = launcher_chunks(B, S)
        bytes_fused = 8 * B * n * nq + PARTIAL_BYTES * 2 * B * chunks + B * (4 * 8 + 4 * 8 + 4)
        bytes_samples = bytes_fused + 2 * 8 * N * nq
        bytes_resident = 8 * N * (2 * nq + nq * nq + 2 * nq) + 8 * N * (nq * nq + 2 * nq + nq)
        med = {k: float(np.median(x)) for k, x in t.items()}
        line = {"bench": "trajectory dynamics, fp64, 16 control points, nq 15", "curves": B, "samples": S,
                "calls_per_window": calls, "is": "seconds per call",
                "fused_s": stats(t["fused"]), "fused_samples_s": stats(t["fused+samples"]),
                "composed_resident_s": stats(t["composed_resident"]),
                "composed_s": stats(t["composed"]), "composed_curves": b,
                "composed_resident_over_fused_samples": med["composed_resident"] / med["fused+samples"],
                "composed_per_curve_over_fused_per_curve": (med["composed"] / b) / (med["fused+samples"] / B),
                "bytes": {"fused": bytes_fused, "fused+samples": bytes_samples, "composed_resident": bytes_resident},
                "GB_per_s": {"fused": bytes_fused / med["fused"] / 1e9,
                             "fused+samples": bytes_samples / med["fused+samples"] / 1e9,
                             "composed_resident": bytes_resident / med["composed_resident"] / 1e9},
                "max_tau_difference": float(np.abs(f["tau"][:b] - g["tau"]).max()),
                "max_g_difference": float(np.abs(f["g"][:b] - g["g"]).max()),
                "max_ratio_difference": float(max(np.abs(f[k][:b] - g[k]).max()
                                                  for k in ("speed_scale", "torque_use", "static_use"))),
                "reductions_equal_samples_run": bool(all(
                    np.array_equal(last["fused"][k].cpu().numpy(), f[k]) for k in last["fused"]))}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)


if __name__ == "__main__":
    main()
