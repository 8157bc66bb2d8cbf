"""Fixtures of the RRT-Connect planner (tests/test_rrt.py, tests/test_gpu_rrt.py)
-> tests/golden/rrt_cases.npz, answered by tests/rrt_oracle.py over
oracle/planner_oracle.py.  Minutes of CPU (the oracle costs 2-50 s per planner
iteration), so the cases are small.

  M  cube from planner_cases sample_t[0] to sample_t[1], qinit / qgoal the
     oracle's cold-start IK of the two ends, the reference's constants,
     RandomState seeds 3, 4 and 6.  Per seed and iteration: bias flag, sample,
     nearest indices, both projected segments, connect distance; both trees
     (parents, q, cube translations); the returned path; the next draw.
  R  the reference's CUBE_PLACEMENT -> CUBE_PLACEMENT_TARGET, seed 0,
     max_iterations=3, max_retries=1: no path; the trees.
  interp_*  SE3.Interpolate at relative rotation angles {0, 1e-5, 2e-4, 1, 3}
     and alpha {0, 0.3, 1}: planner_oracle.se3_interpolate, the same in
     50-digit arithmetic, and the float64 restatement's error against it.
  proj_status  status (0 reached, 1 placement collision, 2 failed IK) of the
     chains `path` and `pathb` of planner_cases.npz.

Asserted for every recorded case (a seed that breaks one is replaced):
  * every nearest-neighbour margin between distinct q values is >= 1e-6;
  * every |dt| / step_size is >= 1e-6 away from an integer (or exactly 0:
    bitwise-equal ends);
  * every connect distance is >= 1e-3 away from the tolerance 0.5;
  * the kdtree and lowest-index runs return the same path once consecutive
    equal rows are removed.

python tests/golden/make_rrt_golden.py
"""
import json
import os
import sys
import warnings
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP, TOL = 0.025, 0.5
M_SEEDS = (3, 4, 6)
ANGLES = (0.0, 1e-5, 2e-4, 1.0, 3.0)
ALPHAS = (0.0, 0.3, 1.0)


def _scene():
    from oracle import collision_oracle as co
    return co.load_scene(os.path.join(HERE, "collision_scene.json"))


def _ends(case):
    pc = np.load(os.path.join(HERE, "planner_cases.npz"))
    kat = json.load(open(os.path.join(HERE, "kat.json")))
    if case == "M":
        return pc["sample_t"][0], pc["sample_t"][1]
    return np.array(kat["cube_placement"]["t"]), np.array(kat["cube_placement_target"]["t"])


def _run(job):
    warnings.filterwarnings("ignore")
    import rrt_oracle
    from oracle import collision_oracle as co
    from oracle import ik_oracle as o
    case, seed, nn = job
    sc = _scene()
    t0, t1 = _ends(case)
    I = np.eye(3)
    qinit, ok0, _, _ = co.computeqgrasppose(sc, np.zeros(o.NQ), I, t0)
    qgoal, ok1, _, _ = co.computeqgrasppose(sc, np.zeros(o.NQ), I, t1)
    assert ok0 and ok1
    kw = dict(max_iterations=3, max_retries=1) if case == "R" else {}
    rs = np.random.RandomState(seed)
    path, trees, log = rrt_oracle.computepath(sc, rs, qinit, qgoal, (I, t0), (I, t1), step_size=STEP,
                                              goal_tolerance=TOL, nn=nn, **kw)
    return dict(case=case, seed=seed, nn=nn, qinit=qinit, qgoal=qgoal, t0=t0, t1=t1, path=path, trees=trees, log=log,
                next=rs.random_sample())


def _check(r):
    for it in r["log"]:
        for m in (it["margin_start"], it["margin_goal"]):
            assert m is None or m >= 1e-6, ("nearest-neighbour margin", r["case"], r["seed"], m)
        for a, b in ((it["from_start_t"], it["t_rand"]), (it["from_goal_t"], r["t1"])):
            x = np.linalg.norm(a - b) / STEP
            # (a projection onto its own start, e.g. the goal tree's root towards the
            # goal, has bitwise-equal ends: exactly 0 in any arithmetic, one step)
            assert x == 0.0 or abs(x - round(x)) >= 1e-6, ("step count", r["case"], r["seed"], x)
        assert abs(it["connect"] - TOL) >= 1e-3, ("connect distance", r["case"], r["seed"], it["connect"])


def _ragged(rows):
    return np.concatenate(rows), np.array([len(x) for x in rows], dtype=np.int64)


def _pack(prefix, r, out):
    log = r["log"]
    out[f"{prefix}_bias"] = np.array([it["bias"] for it in log])
    out[f"{prefix}_q_rand"] = np.array([it["q_rand"] for it in log])
    out[f"{prefix}_t_rand"] = np.array([it["t_rand"] for it in log])
    out[f"{prefix}_near"] = np.array([[it["near_start"], it["near_goal"]] for it in log], dtype=np.int64)
    out[f"{prefix}_connect"] = np.array([it["connect"] for it in log])
    margins = [m for it in log for m in (it["margin_start"], it["margin_goal"]) if m is not None]
    out[f"{prefix}_min_margin"] = np.array(min(margins) if margins else np.nan)
    for side in ("start", "goal"):
        out[f"{prefix}_seg_{side}_q"], out[f"{prefix}_seg_{side}_n"] = _ragged([it[f"seg_{side}_q"] for it in log])
        out[f"{prefix}_seg_{side}_t"], _ = _ragged([it[f"seg_{side}_t"] for it in log])
    G_start, G_cube_start, G_goal, G_cube_goal = r["trees"]
    for side, G, Gc in (("start", G_start, G_cube_start), ("goal", G_goal, G_cube_goal)):
        out[f"{prefix}_{side}_parent"] = np.array([-1 if g[0] is None else g[0] for g in G], dtype=np.int64)
        out[f"{prefix}_{side}_q"] = np.array([g[1] for g in G])
        out[f"{prefix}_{side}_t"] = np.array([g[1][1] for g in Gc])
    out[f"{prefix}_path"] = np.array(r["path"]).reshape(-1, len(r["qinit"]))
    out[f"{prefix}_next"] = np.array(r["next"])


# ---------------------------------------------------------------- SE3.Interpolate in 50 digits (tests/se3_oracle.py)
def make_interp(out):
    from scipy.spatial.transform import Rotation
    from oracle import planner_oracle as po
    from se3_oracle import interpolate_mp
    rng = np.random.default_rng(31)
    rows = []
    for k, ang in enumerate(ANGLES):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        Ra = np.eye(3) if ang == 0.0 else Rotation.random(random_state=40 + k).as_matrix()
        ta, dt = rng.uniform(-0.5, 1.0, 3), rng.uniform(-0.3, 0.3, 3)
        Rb = Ra @ Rotation.from_rotvec(ang * axis).as_matrix() if ang else Ra.copy()
        A, B = (Ra, ta), (Rb, ta + Ra @ dt)
        for al in ALPHAS:
            R, t = po.se3_interpolate(A, B, al)
            f64 = np.concatenate([R.reshape(9), t])
            exact = interpolate_mp(A, B, al)
            rows.append((ang, al, np.concatenate([Ra.reshape(9), ta]), np.concatenate([Rb.reshape(9), B[1]]), f64,
                         exact, np.abs(f64 - exact).max()))
    for i, name in enumerate(("angle", "alpha", "A", "B", "oracle", "exact", "err")):
        out[f"interp_{name}"] = np.array([r[i] for r in rows])
    print("interpolation: float64 restatement error per angle",
          {a: float(max(r[6] for r in rows if r[0] == a)) for a in ANGLES})


def make_proj_status(out):
    from oracle import planner_oracle as po
    pc = np.load(os.path.join(HERE, "planner_cases.npz"))
    sc = _scene()
    status = []
    for key in ("path", "pathb"):
        a, b, n = pc[f"{key}_start_t"], pc[f"{key}_goal_t"], len(pc[f"{key}_q"])
        steps = int(np.linalg.norm(a - b) / STEP) + 1
        if n == steps + 1:
            status.append(0)
            continue
        # the fixture's chain stopped at step n: by the placement check or by the IK
        R, t = po.se3_interpolate((np.eye(3), a), (np.eye(3), b), n / steps)
        status.append(1 if po.target_env(sc, R, t) else 2)
    out["proj_status"] = np.array(status, dtype=np.int32)
    print("projection status (path, pathb):", status)


def main():
    warnings.filterwarnings("ignore")
    out = {}
    make_interp(out)
    make_proj_status(out)
    jobs = [("M", s, nn) for s in M_SEEDS for nn in ("lowest", "kdtree")] + [("R", 0, "lowest"), ("R", 0, "kdtree")]
    with Pool(min(8, len(jobs))) as p:
        res = {(r["case"], r["seed"], r["nn"]): r for r in p.map(_run, jobs)}
    import rrt_oracle
    for (case, seed, nn), r in res.items():
        _check(r)
        if nn == "kdtree":
            a, b = rrt_oracle.dedup(r["path"]), rrt_oracle.dedup(res[(case, seed, "lowest")]["path"])
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), ("kdtree path", case, seed)
    m = res[("M", M_SEEDS[0], "lowest")]
    out.update(M_qinit=m["qinit"], M_qgoal=m["qgoal"], M_t0=m["t0"], M_t1=m["t1"], M_seeds=np.array(M_SEEDS))
    for s in M_SEEDS:
        r = res[("M", s, "lowest")]
        assert len(r["path"]) > 0, ("M did not connect", s)
        _pack(f"M{s}", r, out)
        print(f"M seed {s}: connects at iteration {len(r['log']) - 1}, bias {[it['bias'] for it in r['log']]}, "
              f"min margin {float(out[f'M{s}_min_margin']):.2e}, path {len(r['path'])} rows")
    r = res[("R", 0, "lowest")]
    assert r["path"] == [] and len(r["log"]) == 3
    out.update(R_qinit=r["qinit"], R_qgoal=r["qgoal"], R_t0=r["t0"], R_t1=r["t1"])
    _pack("R", r, out)
    print(f"R: tree sizes {len(r['trees'][0])} / {len(r['trees'][2])}, min margin {float(out['R_min_margin']):.2e}")
    np.savez_compressed(os.path.join(HERE, "rrt_cases.npz"), **out)
    print("wrote rrt_cases.npz")


if __name__ == "__main__":
    main()
