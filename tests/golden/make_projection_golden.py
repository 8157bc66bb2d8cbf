"""Fixture of the device-side path projection (tests/test_projection.py,
tests/test_gpu_projection.py, shared code in tests/projection_cases.py)
-> tests/golden/projection_cases.npz, answered by oracle/planner_oracle.py's
project_path restated here with a trace (the per-solve errors and update
counts it does not return).  A minute or two of CPU on 8 processes: a failing
oracle solve costs 30-50 s, so the chains run in a Pool.

Every chain runs on tests/golden/collision_scene.json.  q0, t0 are
planner_cases.npz path_start_q / path_start_t, tg its path_goal_t; the start
rotation is I.

  zero      I -> I, goal t0 (zero length: one step onto the start)
  short     I -> I, goal t0 + (0.01, 0, 0)
  obst      I -> I, goal (0.43, -0.1, 1.0) (into the obstacle)
  obst_rz   I -> Rz(0.1), the same goal
  far       I -> I, goal (0.95, t0.y, 1.2) (out of reach: the longest chain)
  up, down  I -> I, goal t0 +- (0, 0, 0.06)
  rz        I -> Rz(-0.15), goal tg
  ryrz      I -> Ry(0.05) Rz(0.05), goal tg
  half      I -> Ry(-0.04) Rz(-0.08), goal (t0 + tg) / 2
  spin_m/p  I -> Rz(-+0.05), goal t0 (pure rotations: one step whatever the angle)
  path, pathb   the two chains of planner_cases.npz (pathb's row 0 is robot.q0:
            in collision and no solution of its placement)
  b1, b4, b4s   the step-boundary group, step_size 2^-5, start (0.34375,
            -0.03125, 1.09375), its q the oracle's solve from q0: the goal
            differs on one axis by k 2^-5, k = 1 (x) and 4 (-y), so |dt| /
            step_size is the integer k in any evaluation order; b4s is b4 with
            the distance scaled by (1 - 2^-41): the device counts 4 steps, a
            host that allows for a last-bit difference enqueues 5.

Recorded per chain: the inputs, steps, n_nodes, status (0 reached, 1 placement
collision, 2 failed IK), the oracle's robot_path rows, the update count of
every solve it ran, the cube rows of tests/se3_oracle.py's 50-digit
interpolation, the float64 restatement's rows and its error against those.

Asserted (a candidate that breaks one is replaced, and named here: none so far):
  * every status 0 / 1 / 2 is there; a status-1 and a status-2 chain with
    n_nodes >= 3; a rotated chain of status 0 and of status 1; both pure rotations;
  * outside the boundary group |dt| / step_size is >= 1e-9 from an integer
    (or exactly 0); inside, it is the integer k exactly (b4s: within 1e-11 below);
  * every deciding placement check (each accepted step's "free", the stop of a
    status-1 chain) answers the same on the scene inflated and deflated by 1e-9;
  * every accepted solve stops with its larger hand error below eps (1 - 1e-6),
    collision-free on the inflated scene too, and the iterate before it has
    the error above eps (1 + 1e-6) (or, below eps (1 - 1e-6), collides on the
    deflated scene too);
  * every failing solve also fails at max_iters = 1100, and its iterate 1000
    has a hand error >= 2 eps or collides on the deflated scene too.

python tests/golden/make_projection_golden.py           write the fixture
python tests/golden/make_projection_golden.py --check   regenerate and compare every array bit for bit
"""
import math
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

STEP, BSTEP = 0.025, 2.0 ** -5
B_START = (0.34375, -0.03125, 1.09375)
EPS, MAX_ITERS, LONG_ITERS, DELTA, TIE = 1e-3, 1000, 1100, 1e-9, 1e-6
OUT = os.path.join(HERE, "projection_cases.npz")


def rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def ry(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def chains():
    """[(name, q0 or None (solve the start from planner_cases' q0), start t, goal R, goal t, step_size, k)]"""
    pc = np.load(os.path.join(HERE, "planner_cases.npz"))
    q0, t0, tg = pc["path_start_q"], pc["path_start_t"], pc["path_goal_t"]
    I = np.eye(3)
    obst = np.array([0.43, -0.1, 1.0])
    bs = np.array(B_START)
    out = [
        ("zero", q0, t0, I, t0.copy(), STEP, -1),
        ("short", q0, t0, I, t0 + np.array([0.01, 0.0, 0.0]), STEP, -1),
        ("obst", q0, t0, I, obst, STEP, -1),
        ("obst_rz", q0, t0, rz(0.1), obst, STEP, -1),
        ("far", q0, t0, I, np.array([0.95, t0[1], 1.2]), STEP, -1),
        ("up", q0, t0, I, t0 + np.array([0.0, 0.0, 0.06]), STEP, -1),
        ("down", q0, t0, I, t0 + np.array([0.0, 0.0, -0.06]), STEP, -1),
        ("rz", q0, t0, rz(-0.15), tg, STEP, -1),
        ("ryrz", q0, t0, ry(0.05) @ rz(0.05), tg, STEP, -1),
        ("half", q0, t0, ry(-0.04) @ rz(-0.08), (t0 + tg) / 2, STEP, -1),
        ("spin_m", q0, t0, rz(-0.05), t0.copy(), STEP, -1),
        ("spin_p", q0, t0, rz(0.05), t0.copy(), STEP, -1),
        ("path", q0, t0, I, tg, STEP, -1),
        ("pathb", pc["pathb_start_q"], pc["pathb_start_t"], I, pc["pathb_goal_t"], STEP, -1),
        ("b1", None, bs, I, bs + np.array([BSTEP, 0.0, 0.0]), BSTEP, 1),
        ("b4", None, bs, I, bs + np.array([0.0, -4 * BSTEP, 0.0]), BSTEP, 4),
        ("b4s", None, bs, I, bs + np.array([0.0, -4 * BSTEP * (1.0 - 2.0 ** -41), 0.0]), BSTEP, 4),
    ]
    return out


_SC = {}


def _scene(delta=0.0):
    from oracle import collision_oracle as co
    if delta not in _SC:
        sc = co.load_scene(os.path.join(HERE, "collision_scene.json"))
        if delta:  # make_golden.py _scaled
            for g in sc["geoms"]:
                g["dims"] = np.maximum(g["dims"] + delta * (g["dims"] > 0), 0.0)
        _SC[delta] = sc
    return _SC[delta]


def solve_traced(q0, R, t, max_iters):
    """collision_oracle.computeqgrasppose with the larger hand error of every
    iterate -> (q, ok, it, errs, the iterate before the stop); a solve that
    never stops returns the iterate after MAX_ITERS updates"""
    from oracle import collision_oracle as co
    from oracle import ik_oracle as o
    sc = _scene()
    placements = o.joint_placements()
    L, Rr = o.hook_targets(R, t)
    q = np.array(q0, dtype=np.float64).copy()
    errs, prev = [], None
    for it in range(max_iters):
        eL, eR = o.hand_errors(q, L, Rr, placements)
        nL, nR = np.linalg.norm(eL), np.linalg.norm(eR)
        errs.append(max(nL, nR))
        if nL < EPS and nR < EPS and not co.collision(sc, q, R, t):
            return q, True, it, errs, prev
        JL = o.frame_jacobian_local(q, o.FRAME_LEFT, placements)
        JR = o.frame_jacobian_local(q, o.FRAME_RIGHT, placements)
        vq = np.linalg.pinv(np.vstack([JL, JR])) @ np.hstack([eL, eR])
        prev = q
        q = np.minimum(np.maximum(o.LOWER, q + vq * o.DT), o.UPPER)
        if it + 1 == MAX_ITERS:
            at_max = q.copy()
    return at_max, False, MAX_ITERS, errs, None


def env3(R, t):
    from oracle import planner_oracle as po
    return [bool(po.target_env(_scene(d), R, t)) for d in (0.0, DELTA, -DELTA)]


def _run(ch):
    warnings.filterwarnings("ignore")
    from oracle import collision_oracle as co
    from oracle import planner_oracle as po
    from se3_oracle import interpolate_mp
    name, q0, ta, Rb, tb, step_size, k = ch
    I = np.eye(3)
    if q0 is None:  # the boundary group's start: the oracle's solve from planner_cases' q0
        pc = np.load(os.path.join(HERE, "planner_cases.npz"))
        q0, ok, _, _ = co.computeqgrasppose(_scene(), pc["path_start_q"], I, ta)
        assert ok, (name, "start")
    A, B = (I, np.asarray(ta, dtype=np.float64)), (np.asarray(Rb), np.asarray(tb, dtype=np.float64))
    quot = float(np.linalg.norm(A[1] - B[1]) / step_size)
    steps = int(quot) + 1
    rows, cube64, cube50, iters, acc_err, status = [np.asarray(q0, dtype=np.float64)], [], [], [], [], 0
    a12 = np.concatenate([A[0].reshape(9), A[1]])
    cube64.append(a12), cube50.append(a12)  # row 0 is the input itself
    fail_err, fail_col = np.nan, False
    for s in range(1, steps + 1):
        P = po.se3_interpolate(A, B, s / steps)
        hit = env3(P[0], P[1])
        assert hit[0] == hit[1] == hit[2], (name, s, "placement check near a contact", hit)
        if hit[0]:
            status = 1
            break
        q, ok, it, errs, prev = solve_traced(rows[-1], P[0], P[1], LONG_ITERS)
        iters.append(it)
        if not ok:
            status = 2
            assert len(errs) == LONG_ITERS, (name, s)  # no stop up to 1100 either
            fail_err = float(errs[MAX_ITERS])
            fail_col = bool(co.collision(_scene(-DELTA), q, P[0], P[1]))
            assert co.collision(_scene(), q, P[0], P[1]) == fail_col, (name, s, "collision near a contact")
            assert fail_err >= 2 * EPS or fail_col, (name, s, "near miss", fail_err)
            break
        assert it < MAX_ITERS, (name, s, "stopped between 1000 and 1100 updates", it)
        assert errs[-1] < EPS * (1 - TIE), (name, s, "near tie at the stop", errs[-1])
        assert not co.collision(_scene(DELTA), q, P[0], P[1]), (name, s, "stop near a contact")
        if it > 0:
            assert errs[-2] > EPS * (1 + TIE) or (errs[-2] < EPS * (1 - TIE) and co.collision(_scene(-DELTA), prev, P[0], P[1])), \
                (name, s, "near tie before the stop", errs[-2])
        acc_err.append((errs[-1], errs[-2] if it > 0 else np.nan))
        rows.append(q)
        cube64.append(np.concatenate([P[0].reshape(9), P[1]]))
        cube50.append(interpolate_mp(A, B, s / steps))
    return dict(name=name, q0=rows[0], A=a12, B=np.concatenate([B[0].reshape(9), B[1]]), step=step_size, k=k, quot=quot,
                steps=steps, status=status, rows=np.array(rows), cube64=np.array(cube64), cube50=np.array(cube50),
                iters=np.array(iters, dtype=np.int32), acc_err=np.array(acc_err).reshape(-1, 2), fail_err=fail_err,
                fail_col=fail_col)


def build():
    warnings.filterwarnings("ignore")
    with Pool(min(8, len(chains()))) as p:
        res = p.map(_run, chains(), chunksize=1)
    rot = np.array([not np.array_equal(r["B"][:9], np.eye(3).reshape(9)) for r in res])
    pure = np.array([bool(rot[i]) and np.array_equal(r["A"][9:], r["B"][9:]) for i, r in enumerate(res)])
    st = np.array([r["status"] for r in res], dtype=np.int32)
    nn = np.array([len(r["rows"]) for r in res], dtype=np.int32)
    k = np.array([r["k"] for r in res], dtype=np.int32)
    print(f"{'chain':8s} {'step':>8s} {'quot':>22s} steps nodes status  updates per solve")
    for i, r in enumerate(res):
        print(f"{r['name']:8s} {r['step']:8.5f} {r['quot']:22.15f} {r['steps']:5d} {nn[i]:5d} {st[i]:6d}  {r['iters'].tolist()}")
    # the coverage conditions
    assert set(st) == {0, 1, 2}
    assert ((st == 1) & (nn >= 3)).any() and ((st == 2) & (nn >= 3)).any()
    assert (rot & (st == 0) & ~pure).any() and (rot & (st == 1)).any()
    assert sorted(st[pure]) == [0, 2] and all(r["steps"] == 1 for i, r in enumerate(res) if pure[i])
    for i, r in enumerate(res):
        x = r["quot"]
        if k[i] < 0:
            assert x == 0.0 or abs(x - round(x)) >= 1e-9, ("step count", r["name"], x)
        elif r["name"].endswith("s"):
            assert 0 < k[i] - x < 1e-11 and r["steps"] == k[i] and st[i] == 0, ("spare step", r["name"], x)
            # what a host that divides by step_size (1 - 1e-12) enqueues: one step more
            assert int(np.linalg.norm(r["A"][9:] - r["B"][9:]) / (r["step"] * (1.0 - 1e-12))) + 1 == k[i] + 1
        else:
            assert x == float(k[i]) and r["steps"] == k[i] + 1 and st[i] == 0, ("step boundary", r["name"], x)
    print("conditions hold: statuses", {int(s): int((st == s).sum()) for s in (0, 1, 2)}, "| rotated", int(rot.sum()),
          "| pure rotations", int(pure.sum()), "| placement checks and solves robust at 1e-9 / 1e-6 | failing solves:",
          {r["name"]: (round(r["fail_err"], 6), r["fail_col"]) for r in res if r["status"] == 2})
    cube_err = np.concatenate([np.abs(r["cube64"] - r["cube50"]).max(axis=1) for r in res])
    print("float64 restatement against 50 digits: largest cube-row error", float(cube_err.max()))
    off = lambda key: np.concatenate([[0], np.cumsum([len(r[key]) for r in res])]).astype(np.int64)
    return dict(
        names=np.array([r["name"] for r in res]), q0=np.array([r["q0"] for r in res]), A=np.array([r["A"] for r in res]),
        B=np.array([r["B"] for r in res]), step_size=np.array([r["step"] for r in res]), k=k,
        quot=np.array([r["quot"] for r in res]), steps=np.array([r["steps"] for r in res], dtype=np.int32), n_nodes=nn,
        status=st, rotated=rot, pure_rotation=pure, row_off=off("rows"), q=np.concatenate([r["rows"] for r in res]),
        cube_exact=np.concatenate([r["cube50"] for r in res]), cube_oracle=np.concatenate([r["cube64"] for r in res]),
        cube_err=cube_err, iters_off=off("iters"), iters=np.concatenate([r["iters"] for r in res]),
        acc_off=off("acc_err"), acc_err=np.concatenate([r["acc_err"] for r in res]),
        fail_err=np.array([r["fail_err"] for r in res]), fail_col=np.array([r["fail_col"] for r in res]))


def main():
    out = build()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for key in out:
            assert old[key].dtype == out[key].dtype and old[key].tobytes() == out[key].tobytes(), key
        print("projection_cases.npz reproduces bit for bit:", len(out), "arrays")
        return
    np.savez_compressed(OUT, **out)
    print("wrote projection_cases.npz")


if __name__ == "__main__":
    main()
