"""Fixture of the trajectory check (tests/test_trajcheck.py,
tests/test_gpu_trajcheck.py, shared code in tests/trajcheck_cases.py)
-> tests/golden/trajcheck_cases.npz, answered per sample by the CPU oracles
only: oracle/ik_oracle.py (FK, hook targets, hand_errors),
oracle/collision_oracle.py (colliding_pairs), oracle/planner_oracle.py
(distance_to_obstacle) and tests/rollout_oracle.py's Horner.  Grasp
configurations come from the C oracle (oracle/c_oracle.py, the IK with the
collision term), fitted curves from tests/fit_oracle.py.  A minute or two of
CPU on 8 processes.

Every curve runs on tests/golden/collision_scene.json, mult = 1, t_min = 0.
A = CUBE_PLACEMENT, B = CUBE_PLACEMENT_TARGET (config.py), qA / qB their grasps.

  group fit   n_points 21, S 33, t_max 15, cube carried
    free      the degree-20 fit through 23 via-grasps: lift A to z = 1.1, cross, lower onto B
    limit     free with control points 8 .. 12 of HEAD_JOINT0 raised by 2 rad: the
              head leaves its limit in the interior, nothing collides
  group line  n_points 3, S 17, t_max 1, carried
    line      the straight joint-space line qA -> qB (the connect jump's shape)
  group trio  n_points 3, S 9, t_max 1, carried: one batch, the free curve between the other two
    from0     robot.q0 -> qA: collides from sample 0
    short     via-grasp 8 -> via-grasp 9 (free)
    last      qA -> line(e): only the last sample collides, robustly; e the first of
              1/100, 1/104 .. 1/124 that gives it (the line's first contact is near u = 0.009)
  group fixed n_points 3, S 9, t_max 1, cube FIXED at A
    reach     robot.q0 -> qA: the grasp error falls below EPSILON at the last sample
  group two   n_points 3, S 2, t_max 1, carried
    ends      the line's control points: its two end samples alone

Recorded per sample: q, the cube placement, collision, the lowest colliding
pair, whether a hand-cube pair collides, clearance, grasp, limit, and `robust`:
the collision flag is the same with every shape grown and shrunk by 1e-6 m.
Per curve: the folds, pin_pair (the lowest colliding pair at the first
collision is the same on the grown and shrunk scenes) and pin_count (every
sample robust).  dev_grasp / dev_limit / dev_cube: the float64 oracle's largest
deviation from the same samples evaluated in 32 digits (mpmath).

Also stored: the 23 via-grasps (`via`; the fit test's path and the polyline of
the path test: via 2 -> via 1 -> via 1 -> qA -> qB, free before the jump).

Asserted (conditions 1-8 of the fixture's specification):
  1 free: no collision, clearance > 0 at every sample;
  2 line: sample 0 free, first collision strictly inside, its first_pair an
    arm-obstacle pair, some sample's colliding set holds a hand-cube pair;
  3 from0 collides at sample 0, last at sample S-1 only, short is free between them;
  4 limit: max_limit > 0 with its arg strictly inside, no collision;
  5 reach: grasp[-1] < EPSILON < grasp[0], non-increasing along the curve;
  6 the S = 2 and n_points = 3 cases are there;
  7 >= 95 % of all samples robust; in every curve the samples up to and including
    the first collision are robust; arg-min clearance unique by > 1e-6 where the
    minimum is compared (> 1e-6), arg-max grasp and limit by > 1e-9;
  8 the 32-digit deviations are recorded (the tests bound at 16 x, floored at 1e-12).

python tests/golden/make_trajcheck_golden.py           write the fixture
python tests/golden/make_trajcheck_golden.py --check   regenerate and compare every array bit for bit
"""
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

import trajcheck_cases as tc  # noqa: E402

OUT = os.path.join(HERE, "trajcheck_cases.npz")
A = np.array([0.33, -0.3, 0.93])
B = np.array([0.4, 0.11, 0.93])
LIFT_Z, DELTA, DPS = 1.1, 1e-6, 32
LAST_ENDS = tuple(1.0 / d for d in range(100, 128, 4))
HAND_JOINTS = (8, 14)  # LARM_JOINT5, RARM_JOINT5: the links that carry the hand geometries
ARM_JOINTS = range(3, 15)
I9 = np.eye(3).reshape(9)


def placement(t):
    return np.concatenate([I9, np.asarray(t, dtype=np.float64)])


def via_grasps():
    """23 grasps warm-started along lift / cross / lower (the C oracle's IK with the collision term)"""
    from oracle import c_oracle
    sc = tc.oracle_scene()
    leg = lambda a, b, n: [a + (b - a) * k / n for k in range(1, n + 1)]
    Au, Bu = A + [0, 0, LIFT_Z - A[2]], B + [0, 0, LIFT_Z - B[2]]
    q, out = np.zeros(15), []
    for t in [A] + leg(A, Au, 6) + leg(Au, Bu, 10) + leg(Bu, B, 6):
        qq, ok, _, _ = c_oracle.solve_collision(sc, placement(t)[None], q)
        assert ok[0], ("via grasp", t)
        q = qq[0]
        out.append(q)
    return np.array(out)


def line3(a, b):
    return np.stack([a, (a + b) / 2, b])


# ---------------------------------------------------------------- one sample, float64 and 32 digits
def _sample(args):
    """-> dict of one sample by the oracles (a Pool worker)"""
    warnings.filterwarnings("ignore")
    from oracle import c_oracle
    from oracle import collision_oracle as co
    from oracle import planner_oracle as po
    points, t_max, t, fixed = args
    sc = tc.oracle_scene()
    q = tc.curve_value(points, 0.0, t_max, 1.0, t)
    cube, grasp, limit = tc.kinematic_sample(q, fixed)
    R, tt = cube[:9].reshape(3, 3), cube[9:]
    hits = co.colliding_pairs(sc, q, R, tt)
    idx = sorted(sc["pairs"].index(p) for p in hits)
    flags = [bool(c_oracle.collision(tc.oracle_scene(d), q[None], cube[None])[0]) for d in (0.0, DELTA, -DELTA)]
    assert flags[0] == bool(idx), "the C and the Python collision oracles disagree"
    tgt = next(i for i, g in enumerate(sc["geoms"]) if g["target"])
    hand_cube = any(tgt in p and sc["geoms"][p[0] if p[1] == tgt else p[1]]["joint"] in HAND_JOINTS for p in hits)
    low = [-1, -1]  # the lowest colliding pair on the grown and on the shrunk scene
    if idx:
        for k, d in enumerate((DELTA, -DELTA)):
            h = co.colliding_pairs(tc.oracle_scene(d), q, R, tt)
            low[k] = min(tc.oracle_scene(d)["pairs"].index(p) for p in h) if h else -1
    mq, mcube, mgrasp, mlimit = sample_mp(points, t_max, t, fixed)
    return dict(q=q, cube=cube, grasp=grasp, limit=limit, collision=bool(idx), first_pair=idx[0] if idx else -1,
                hand_cube=hand_cube, robust=flags[0] == flags[1] == flags[2], low=low,
                clearance=po.distance_to_obstacle(sc, q, R, tt),
                dev=(abs(grasp - mgrasp), abs(limit - mlimit), float(np.abs(cube - mcube).max())))


def sample_mp(points, t_max, t, fixed):
    """The same sample in DPS digits from the float64 inputs -> (q, cube [12], grasp, limit) rounded to float64"""
    import mpmath as mp

    from oracle import ik_oracle as ik
    mp.mp.dps = DPS
    f = mp.mpf
    mat = lambda M: [[f(float(M[i][j])) for j in range(3)] for i in range(3)]
    vec = lambda v: [f(float(x)) for x in v]
    mm = lambda X, Y: [[X[i][0] * Y[0][j] + X[i][1] * Y[1][j] + X[i][2] * Y[2][j] for j in range(3)] for i in range(3)]
    mv = lambda X, v: [X[i][0] * v[0] + X[i][1] * v[1] + X[i][2] * v[2] for i in range(3)]
    mtv = lambda X, v: [X[0][i] * v[0] + X[1][i] * v[1] + X[2][i] * v[2] for i in range(3)]
    tr = lambda X: [[X[j][i] for j in range(3)] for i in range(3)]
    se3 = lambda X, Y: (mm(X[0], Y[0]), [X[1][i] + mv(X[0], Y[1])[i] for i in range(3)])
    inv = lambda X: (tr(X[0]), [-x for x in mtv(X[0], X[1])])

    def rot(axis, a):
        s, c, o, z = mp.sin(a), mp.cos(a), f(1), f(0)
        if axis == 0:
            return [[o, z, z], [z, c, -s], [z, s, c]]
        if axis == 1:
            return [[c, z, s], [z, o, z], [-s, z, c]]
        return [[c, -s, z], [s, c, z], [z, z, o]]

    # Bezier.__call__ (control.py:30-46)
    P = [[f(float(x)) for x in row] for row in points]
    n = len(P) - 1
    u = f(float(t)) / f(float(t_max))
    uo, bc, tn = 1 - u, f(1), f(1)
    tmp = [x * uo for x in P[0]]
    for i in range(1, n):
        tn = tn * u
        bc = bc * (f(n - i + 1) / f(i))
        tmp = [(a + (tn * bc) * b) * uo for a, b in zip(tmp, P[i])]
    q = [a + (tn * u) * b for a, b in zip(tmp, P[n])]
    pl = [(mat(R0), vec(t0)) for R0, t0 in ik.joint_placements()]
    oMi = []
    for j in range(ik.NQ):
        loc = (mm(pl[j][0], rot(ik.AXIS[j], q[j])), pl[j][1])
        oMi.append(loc if ik.PARENT[j] < 0 else se3(oMi[ik.PARENT[j]], loc))
    hands = [se3(oMi[j], (mat(Rf), vec(tf))) for j, Rf, tf in (ik.FRAME_LEFT, ik.FRAME_RIGHT)]
    hooks = [(mat(H[0]), vec(H[1])) for H in (ik.HOOK_LEFT, ik.HOOK_RIGHT)]
    cube = se3(hands[0], inv(hooks[0])) if fixed is None else (mat(fixed[:9].reshape(3, 3)), vec(fixed[9:]))
    norms = []
    for h in ((1,) if fixed is None else (0, 1)):
        Rh, th = hands[h]
        TR, Tt = se3(cube, hooks[h])
        e = ik.log6_mp(mm(tr(Rh), TR), mtv(Rh, [Tt[i] - th[i] for i in range(3)]))
        norms.append(mp.sqrt(sum(x * x for x in e)))
    lim = max([f(0)] + [q[j] - f(float(ik.UPPER[j])) for j in range(ik.NQ)] +
              [f(float(ik.LOWER[j])) - q[j] for j in range(ik.NQ)])
    flat = [cube[0][i][j] for i in range(3) for j in range(3)] + cube[1]
    return (np.array([float(x) for x in q]), np.array([float(x) for x in flat]), float(max(norms)), float(lim))


# ---------------------------------------------------------------- the curves
def curves():
    """[(name, group, points, fixed placement or None)] and the groups [(name, n_points, S, t_max, fixed)]"""
    via = via_grasps()
    import fit_oracle as fo
    qA, qB, q0 = via[0], via[-1], np.zeros(15)
    free = fo.fit_f64(qA, qB, via, 15.0)
    limit = free.copy()
    limit[8:13, 1] += 2.0
    groups = [("fit", 21, 33, 15.0, False), ("line", 3, 17, 1.0, False), ("trio", 3, 9, 1.0, False),
              ("fixed", 3, 9, 1.0, True), ("two", 3, 2, 1.0, False)]
    out = [("free", 0, free, None), ("limit", 0, limit, None), ("line", 1, line3(qA, qB), None),
           ("from0", 2, line3(q0, qA), None), ("short", 2, line3(via[8], via[9]), None), ("last", 2, None, None),
           ("reach", 3, line3(q0, qA), placement(A)), ("ends", 4, line3(qA, qB), None)]
    return out, groups, (qA, qB, via)


def run_curve(pool, points, S, t_max, fixed):
    ts = tc.sample_times(0.0, t_max, S)
    return pool.map(_sample, [(points, t_max, float(t), fixed) for t in ts], chunksize=1)


def build():
    warnings.filterwarnings("ignore")
    from oracle import planner_oracle as po
    cs, groups, (qA, qB, via) = curves()
    res = {}
    with Pool(8) as pool:
        for k, (name, g, pts, fixed) in enumerate(cs):
            S, t_max = groups[g][2], groups[g][3]
            if name == "last":  # qA -> line(e): the first e whose last sample alone collides, robustly
                for e in LAST_ENDS:
                    pts = line3(qA, qA + (qB - qA) * e)
                    r = run_curve(pool, pts, S, t_max, None)
                    col = [s["collision"] for s in r]
                    if col == [False] * (S - 1) + [True] and all(s["robust"] for s in r):
                        break
                else:
                    raise AssertionError("no end parameter gives a curve that collides at its last sample only")
                print("last: e =", e)
                cs[k] = (name, g, pts, None)
                res[name] = r
            else:
                res[name] = run_curve(pool, pts, S, t_max, fixed)
    sc = tc.oracle_scene()
    out = {k: [] for k in ("q", "cube", "collision", "first_pair_at", "hand_cube", "robust", "clearance", "grasp",
                           "limit")}
    per = {k: [] for k in tc.CURVE + ("pin_pair", "pin_count")}
    dev = np.zeros(3)
    print(f"{'curve':6s} {'S':>3s} first pair  n  robust  min clearance @   max grasp @     max limit @")
    for name, g, pts, fixed in cs:
        r = res[name]
        col = np.array([s["collision"] for s in r])
        arr = lambda key: np.array([s[key] for s in r])
        f = tc.fold(col, arr("first_pair"), arr("clearance"), arr("grasp"), arr("limit"))
        rob = arr("robust")
        fc = f["first_collision"]
        # condition 7, per curve
        assert rob[:fc + 1].all() if fc >= 0 else True, (name, "a sample up to the first collision is near a contact")
        cl = arr("clearance")
        if f["min_clearance"] > tc.CLEAR_MIN:
            assert np.sort(cl)[1] - np.sort(cl)[0] > 1e-6, (name, "arg-min clearance is a near tie")
        gr, li = np.sort(arr("grasp")), np.sort(arr("limit"))
        assert gr[-1] - gr[-2] > 1e-9, (name, "arg-max grasp is a near tie")
        assert f["max_limit"] == 0.0 or li[-1] - li[-2] > 1e-9, (name, "arg-max limit is a near tie")
        pin_pair = fc >= 0 and r[fc]["low"][0] == r[fc]["low"][1] == f["first_pair"]
        for key in tc.CURVE:
            per[key].append(f[key])
        per["pin_pair"].append(bool(pin_pair))
        per["pin_count"].append(bool(rob.all()))
        for key, src in (("q", "q"), ("cube", "cube"), ("collision", "collision"), ("first_pair_at", "first_pair"),
                         ("hand_cube", "hand_cube"), ("robust", "robust"), ("clearance", "clearance"),
                         ("grasp", "grasp"), ("limit", "limit")):
            out[key].append(arr(src))
        dev = np.maximum(dev, np.max([s["dev"] for s in r], axis=0))
        print(f"{name:6s} {len(r):3d} {fc:5d} {f['first_pair']:4d} {f['n_collision']:2d} {int(rob.sum()):3d}/{len(r):<3d} "
              f"{f['min_clearance']:12.6f} {f['arg_clearance']:2d} {f['max_grasp']:12.4e} {f['arg_grasp']:2d} "
              f"{f['max_limit']:10.4e} {f['arg_limit']:2d}")
    by = {name: i for i, (name, _, _, _) in enumerate(cs)}
    col = lambda n: out["collision"][by[n]]
    # 1
    assert not col("free").any() and (out["clearance"][by["free"]] > 0).all()
    # 2
    i = by["line"]
    fc, S = per["first_collision"][i], len(col("line"))
    assert not col("line")[0] and 0 < fc < S - 1
    a, b = sc["pairs"][per["first_pair"][i]]
    assert sc["geoms"][a]["joint"] in ARM_JOINTS and b == po.env_ids(sc)[1]
    assert per["pin_pair"][i] and out["hand_cube"][i].any()
    # 3: neighbours in one batch
    assert [n for n, g, _, _ in cs if g == 2] == ["from0", "short", "last"]
    assert col("from0")[0] and not col("short").any()
    assert col("last").tolist() == [False] * (len(col("last")) - 1) + [True]
    # 4
    i = by["limit"]
    assert per["max_limit"][i] > 0 and 0 < per["arg_limit"][i] < len(col("limit")) - 1 and not col("limit").any()
    # 5
    g = out["grasp"][by["reach"]]
    assert g[-1] < tc.EPSILON < g[0] and (np.diff(g) <= 0).all()
    # 6
    assert len(col("ends")) == 2 and all(len(p) in (3, 21) for _, _, p, _ in cs)
    # the polyline of the path test, via 2 -> via 1 -> via 1 -> qA -> qB at 16 samples per segment: its first two
    # segments are free on the grown scene too, so its first collision is the line's
    from oracle import c_oracle
    for a, b in ((via[2], via[1]), (via[1], via[0])):
        qs = np.array([tc.curve_value(line3(a, b), 0.0, 1.0, 1.0, t) for t in tc.sample_times(0.0, 1.0, 17)])
        cubes = np.array([tc.kinematic_sample(q)[0] for q in qs])
        assert not c_oracle.collision(tc.oracle_scene(DELTA), qs, cubes).any(), "a polyline segment before the jump collides"
    # 7
    rob = np.concatenate(out["robust"])
    assert rob.mean() >= 0.95, rob.mean()
    print("conditions hold | robust samples", int(rob.sum()), "of", rob.size, "| float64 oracle against", DPS,
          "digits: grasp", dev[0], "limit", dev[1], "cube", dev[2])
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    pts = [p for _, _, p, _ in cs]
    return dict(
        names=np.array([n for n, _, _, _ in cs]), group=np.array([g for _, g, _, _ in cs], dtype=np.int32),
        group_names=np.array([g[0] for g in groups]), group_n_points=np.array([g[1] for g in groups], dtype=np.int32),
        group_S=np.array([g[2] for g in groups], dtype=np.int32), group_t_max=np.array([g[3] for g in groups]),
        group_fixed=np.array([g[4] for g in groups]),
        cube_fixed=np.array([np.zeros(12) if f is None else f for _, _, _, f in cs]),
        pt_off=off(pts), points=np.concatenate(pts), s_off=off(out["q"]), q=np.concatenate(out["q"]),
        cube=np.concatenate(out["cube"]), collision=np.concatenate(out["collision"]),
        first_pair_at=np.concatenate(out["first_pair_at"]).astype(np.int32), hand_cube=np.concatenate(out["hand_cube"]),
        robust=rob, clearance=np.concatenate(out["clearance"]), grasp=np.concatenate(out["grasp"]),
        limit=np.concatenate(out["limit"]),
        first_collision=np.array(per["first_collision"], dtype=np.int32),
        first_pair=np.array(per["first_pair"], dtype=np.int32), n_collision=np.array(per["n_collision"], dtype=np.int32),
        min_clearance=np.array(per["min_clearance"]), arg_clearance=np.array(per["arg_clearance"], dtype=np.int32),
        max_grasp=np.array(per["max_grasp"]), arg_grasp=np.array(per["arg_grasp"], dtype=np.int32),
        max_limit=np.array(per["max_limit"]), arg_limit=np.array(per["arg_limit"], dtype=np.int32),
        pin_pair=np.array(per["pin_pair"]), pin_count=np.array(per["pin_count"]),
        pair_idx=np.array(po.obstacle_pairs(sc), dtype=np.int32),
        dev_grasp=np.float64(dev[0]), dev_limit=np.float64(dev[1]), dev_cube=np.float64(dev[2]), qA=qA, qB=qB, via=via)


def main():
    out = build()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for key in out:
            assert old[key].dtype == out[key].dtype and old[key].tobytes() == out[key].tobytes(), key
        print("trajcheck_cases.npz reproduces bit for bit:", len(out), "arrays")
        return
    np.savez_compressed(OUT, **out)
    print("wrote trajcheck_cases.npz")


if __name__ == "__main__":
    main()
