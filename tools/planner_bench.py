"""Planner-row benchmark: the GPU sampler / projection against
the reference-semantics CPU oracle (numpy, oracle/planner_oracle.py).  One
JSON line.  python tools/planner_bench.py [--n 512 --chains 256]

Also: project_paths' host route against its device route (ikg_project_paths)
on the same chains, alternating in one run, --repeats times each; the
lock-step planner `computepaths` at --planners planners on query M
(tests/golden/rrt_cases.npz) in planners per second; the sequential drop-in
`computepath` on the same query.  Each timed call ends with its results on the
host, i.e. after the device has finished."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "motion-planning-and-control-for-dual-manipulator-robot_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="valid samples for the batched sampler")
    ap.add_argument("--chains", type=int, default=256, help="projection chains per batched call")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats of each projection route")
    ap.add_argument("--planners", type=int, default=64, help="lock-step planners of the computepaths timing")
    ap.add_argument("--no-planner", action="store_true")
    ap.add_argument("--only-device-route", action="store_true",
                    help="the sampler, then the device route three times: the run to put under rocprofv3 --kernel-trace")
    a = ap.parse_args()
    import ikgrasp
    from ikgrasp.config import CUBE_PLACEMENT, CUBE_PLACEMENT_TARGET
    from ikgrasp.path import project_path, project_paths, sample_cube_placement, sample_cube_placements
    from ikgrasp.se3 import SE3
    robot, _, _, cube = ikgrasp.setuppinocchio()
    out = {"bench": "planner (SURVEY 8f-2)"}
    # warm-up
    sample_cube_placements(robot, CUBE_PLACEMENT, CUBE_PLACEMENT_TARGET, 8, rng=np.random.default_rng(0), batch=256)
    t0 = time.perf_counter()
    q, t = sample_cube_placements(robot, CUBE_PLACEMENT, CUBE_PLACEMENT_TARGET, a.n, rng=np.random.default_rng(1),
                                  batch=4096)
    dt = time.perf_counter() - t0
    out["batched_sampler"] = {"valid_samples": a.n, "s": dt, "valid_samples_per_s": a.n / dt}
    np.random.seed(0)
    t0 = time.perf_counter()
    for _ in range(8):
        sample_cube_placement(robot, cube, CUBE_PLACEMENT, CUBE_PLACEMENT_TARGET, batch=64)
    out["dropin_sample_cube_placement_ms"] = (time.perf_counter() - t0) / 8 * 1e3
    # projection chains between valid samples
    C = min(a.chains, len(q) - 1)
    starts = [SE3(np.eye(3), t[i]) for i in range(C)]
    goals = [SE3(np.eye(3), t[i + 1]) for i in range(C)]
    if a.only_device_route:
        for _ in range(3):
            paths = project_paths(robot, list(q[:C]), starts, goals, on_device=True)
        print(json.dumps({"bench": "planner device route", "chains": C,
                          "solved_steps": sum(len(p[0]) - 1 for p in paths)}))
        return
    t0 = time.perf_counter()
    for i in range(4):
        project_path(robot, cube, q[i], starts[i], goals[i])
    out["dropin_project_path_ms"] = (time.perf_counter() - t0) / 4 * 1e3
    t0 = time.perf_counter()
    paths = project_paths(robot, list(q[:C]), starts, goals)
    dt = time.perf_counter() - t0
    steps = sum(len(p[0]) - 1 for p in paths)
    out["batched_project_paths"] = {"chains": C, "s": dt, "paths_per_s": C / dt, "solved_steps": steps}
    # host route vs device route on the same chains, alternating (both warm by now / after one call)
    dev_paths = project_paths(robot, list(q[:C]), starts, goals, on_device=True)
    same = all(len(a[0]) == len(b[0]) for a, b in zip(paths, dev_paths))
    dq = max(float(np.abs(np.array(a[0]) - np.array(b[0])).max()) for a, b in zip(paths, dev_paths)) if same else None
    th, td = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        project_paths(robot, list(q[:C]), starts, goals)
        th.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        project_paths(robot, list(q[:C]), starts, goals, on_device=True)
        td.append(time.perf_counter() - t0)
    stat = lambda x: {"ms": [round(v * 1e3, 3) for v in x], "median_ms": float(np.median(x)) * 1e3,
                      "min_ms": min(x) * 1e3, "max_ms": max(x) * 1e3}
    out["project_paths_routes"] = {"chains": C, "solved_steps": steps, "host": stat(th), "device": stat(td),
                                   "speedup_median": float(np.median(th) / np.median(td)),
                                   "same_lengths": same, "max_abs_dq": dq}
    if not a.no_planner:
        from ikgrasp.path import computepath, computepaths
        c = np.load(os.path.join(ROOT, "tests", "golden", "rrt_cases.npz"))
        qi, qg = c["M_qinit"], c["M_qgoal"]
        ca, cb = SE3(np.eye(3), c["M_t0"]), SE3(np.eye(3), c["M_t1"])
        P = a.planners
        computepaths(robot, [qi] * 2, [qg] * 2, [ca] * 2, [cb] * 2, [0, 1])  # warm-up
        t0 = time.perf_counter()
        res = computepaths(robot, [qi] * P, [qg] * P, [ca] * P, [cb] * P, list(range(100, 100 + P)))
        dt = time.perf_counter() - t0
        out["computepaths"] = {"query": "M", "planners": P, "s": dt, "planners_per_s": P / dt,
                               "connected": sum(1 for r in res if len(r))}
        np.random.seed(0)
        computepath(qi, qg, ca, cb, robot=robot, cube=cube)  # warm-up
        t0 = time.perf_counter()
        n, found = 8, 0
        for _ in range(n):
            found += bool(len(computepath(qi, qg, ca, cb, robot=robot, cube=cube)))
        dt = time.perf_counter() - t0
        out["computepath"] = {"query": "M", "calls": n, "connected": found, "s_per_call": dt / n,
                              "planners_per_s": n / dt}
    if not a.no_cpu:
        warnings.filterwarnings("ignore")
        from oracle import collision_oracle as co
        from oracle import planner_oracle as po
        sc = co.load_scene(os.path.join(ROOT, "tests", "golden", "collision_scene.json"))
        rs = np.random.RandomState(0)
        t0 = time.perf_counter()
        po.sample_cube_placement(sc, rs, CUBE_PLACEMENT.translation, CUBE_PLACEMENT_TARGET.translation)
        out["cpu_oracle_sample_cube_placement_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        po.project_path(sc, q[0], (np.eye(3), t[0]), (np.eye(3), t[1]))
        out["cpu_oracle_project_path_ms"] = (time.perf_counter() - t0) * 1e3
        out["cpu_note"] = "numpy restatement (reference-semantics Python loop, 1 core), not Pinocchio"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
