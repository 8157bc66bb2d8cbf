"""Shared code of tests/test_trajcheck.py (host emulator) and
tests/test_gpu_trajcheck.py (ikg_trajectory_check_batch on the GPU): the
fixture tests/golden/trajcheck_cases.npz (tests/golden/make_trajcheck_golden.py),
the per-sample CPU oracle the fixture is answered by, and the comparison with
it (test infrastructure).

A leg gives `run(points [B,n,nq], t_min, t_max, mult, S, cube_fixed [B,12] or
None, pair_idx, samples_per_wave=0)` -> dict of every output of the entry
(numpy): one call with all outputs requested.

The curves form groups, one call each (a call has one n_points, S, range and
cube mode); `group_*` arrays describe them and `group[c]` is curve c's.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPSILON = 1e-3  # config.py:22
CLEAR_TOL, CLEAR_MIN = 1e-7, 1e-6  # ikg_distance_batch's bar (tests/test_gpu_planner.py)
FLOOR = 1e-12
CURVE = ("first_collision", "first_pair", "n_collision", "min_clearance", "arg_clearance", "max_grasp", "arg_grasp",
         "max_limit", "arg_limit")
SAMPLE = ("collision", "clearance", "grasp", "limit", "cube")
NO_CLEARANCE = 1e30

_cache = {}


def cases():
    if "c" not in _cache:
        _cache["c"] = dict(np.load(os.path.join(GOLDEN, "trajcheck_cases.npz")))
    return _cache["c"]


def names():
    return [str(n) for n in cases()["names"]]


def index(name):
    return names().index(name)


def group_names():
    return [str(n) for n in cases()["group_names"]]


def members(g):
    return [i for i, x in enumerate(cases()["group"]) if x == g]


def sample_times(t_min, t_max, S):
    """t_k = t_min + k (t_max - t_min) / (S - 1), t_{S-1} = t_max exactly (the entry's rule, float64)"""
    t = [t_min + (k * (t_max - t_min)) / (S - 1) for k in range(S)]
    t[-1] = t_max
    return np.array(t, dtype=np.float64)


def points_of(i):
    c = cases()
    return c["points"][int(c["pt_off"][i]):int(c["pt_off"][i + 1])]


def samples_of(i, key):
    c = cases()
    return c[key][int(c["s_off"][i]):int(c["s_off"][i + 1])]


def group_inputs(g, idx=None):
    """(points [B,n,nq], t_min, t_max, mult, S, cube_fixed or None) of group g (or of its curves idx)"""
    c = cases()
    idx = members(g) if idx is None else list(idx)
    pts = np.ascontiguousarray(np.stack([points_of(i) for i in idx]))
    fixed = np.ascontiguousarray(c["cube_fixed"][idx]) if c["group_fixed"][g] else None
    return pts, 0.0, float(c["group_t_max"][g]), 1.0, int(c["group_S"][g]), fixed


# ---------------------------------------------------------------- the per-sample oracle (float64)
def curve_value(points, t_min, t_max, mult, t):
    """tests/rollout_oracle.py's Horner in float64"""
    import dynamics_oracle as do
    import rollout_oracle as ro
    return np.asarray(ro.bezier(do.F64, (points, t_min, t_max, mult), float(t)), dtype=np.float64)


def carried_cube(q):
    """oM(LARM_EFF) * hook_L^-1 by oracle/ik_oracle.py -> (R, t)"""
    from oracle import ik_oracle as ik
    hL = ik.frame_placement(ik.forward_kinematics(q), ik.FRAME_LEFT)
    return ik.se3_mul(hL, ik.se3_inv(ik.HOOK_LEFT))


def cube12(M):
    return np.concatenate([np.asarray(M[0]).reshape(9), np.asarray(M[1])])


def kinematic_sample(q, fixed=None):
    """-> (cube [12], grasp, limit): hand_errors' norms at the cube placement
    (CARRIED: the right hand's; FIXED: the larger) and tools.jointlimitscost's excess"""
    from oracle import ik_oracle as ik
    q = np.asarray(q, dtype=np.float64)
    cube = carried_cube(q) if fixed is None else (fixed[:9].reshape(3, 3), fixed[9:])
    L, R = ik.hook_targets(cube[0], cube[1])
    eL, eR = ik.hand_errors(q, L, R)
    grasp = float(np.linalg.norm(eR)) if fixed is None else float(max(np.linalg.norm(eL), np.linalg.norm(eR)))
    limit = float(max(0.0, np.max(q - ik.UPPER), np.max(ik.LOWER - q)))
    return cube12(cube), grasp, limit


def oracle_scene(delta=0.0):
    """tests/golden/collision_scene.json, every shape grown by delta (sphere
    radius, box half-extents, cylinder radius and half-length)"""
    from oracle import collision_oracle as co
    key = ("scene", delta)
    if key not in _cache:
        sc = co.load_scene(os.path.join(GOLDEN, "collision_scene.json"))
        for g in sc["geoms"]:
            g["dims"] = np.maximum(g["dims"] + delta * (g["dims"] > 0), 0.0)
        _cache[key] = sc
    return _cache[key]


# ---------------------------------------------------------------- folds and comparisons
def fold(collision, first_pair_at, clearance, grasp, limit, measured=True):
    """One curve's per-sample arrays -> its per-curve outputs (the lowest sample on ties)"""
    col = np.asarray(collision).astype(bool)
    out = {"first_collision": -1, "first_pair": -1, "n_collision": int(col.sum())}
    if col.any():
        out["first_collision"] = int(np.argmax(col))
        out["first_pair"] = int(first_pair_at[out["first_collision"]]) if first_pair_at is not None else None
    out["arg_clearance"] = int(np.argmin(clearance)) if measured else -1
    out["min_clearance"] = float(np.min(clearance)) if measured else NO_CLEARANCE
    out["arg_grasp"], out["max_grasp"] = int(np.argmax(grasp)), float(np.max(grasp))
    out["arg_limit"], out["max_limit"] = int(np.argmax(limit)), float(np.max(limit))
    return out


def check_self_fold(got, j):
    """Curve j's per-curve outputs of `got` equal the fold of its own per-sample outputs exactly"""
    f = fold(got["collision"][j], None, got["clearance"][j], got["grasp"][j], got["limit"][j],
             measured=got["arg_clearance"][j] >= 0)
    for k in CURVE:
        if k == "first_pair":
            assert (got[k][j] >= 0) == (f["first_collision"] >= 0), (j, k)
        else:
            assert got[k][j] == f[k], (j, k, got[k][j], f[k])


def bounds():
    """test bounds for grasp, limit and cube: 16 x the float64 oracle's largest
    deviation from the 32-digit evaluation, floored at 1e-12"""
    c = cases()
    return {k: max(16.0 * float(c["dev_" + k]), FLOOR) for k in ("grasp", "limit", "cube")}


def compare(i, got, j, verbose=False):
    """Curve j of the answer `got` against fixture curve i under the fixture's bars"""
    c = cases()
    name = names()[i]
    b = bounds()
    robust = samples_of(i, "robust")
    col = samples_of(i, "collision")
    gcol = np.asarray(got["collision"][j]).astype(bool)
    assert np.array_equal(gcol[robust], col[robust]), (name, "collision flags", gcol.tolist(), col.tolist())
    fig = {}
    for key in ("grasp", "limit", "cube"):
        ref = samples_of(i, key)
        fig[key] = float(np.abs(np.asarray(got[key][j]) - ref).max())
    cl = samples_of(i, "clearance")
    cmp_ = cl > CLEAR_MIN
    fig["clearance"] = float(np.abs(np.asarray(got["clearance"][j]) - cl)[cmp_].max()) if cmp_.any() else 0.0
    if verbose:
        print(name, {k: f"{v:.3e}" for k, v in fig.items()}, "bounds", {k: f"{v:.3e}" for k, v in b.items()})
    for key in ("grasp", "limit", "cube"):
        assert fig[key] <= b[key], (name, key, fig[key], b[key])
    assert fig["clearance"] <= CLEAR_TOL, (name, "clearance", fig["clearance"])
    assert int(got["first_collision"][j]) == int(c["first_collision"][i]), (name, int(got["first_collision"][j]))
    if c["pin_pair"][i]:
        assert int(got["first_pair"][j]) == int(c["first_pair"][i]), (name, int(got["first_pair"][j]))
    if c["pin_count"][i]:
        assert int(got["n_collision"][j]) == int(c["n_collision"][i]), (name, int(got["n_collision"][j]))
    # the arg-extremes are unique in the fixture by more than the bounds
    assert int(got["arg_grasp"][j]) == int(c["arg_grasp"][i]), (name, "arg_grasp")
    assert int(got["arg_limit"][j]) == int(c["arg_limit"][i]) or c["max_limit"][i] == 0.0, (name, "arg_limit")
    assert abs(float(got["max_grasp"][j]) - float(c["max_grasp"][i])) <= b["grasp"], (name, "max_grasp")
    assert abs(float(got["max_limit"][j]) - float(c["max_limit"][i])) <= b["limit"], (name, "max_limit")
    if c["min_clearance"][i] > CLEAR_MIN:
        assert int(got["arg_clearance"][j]) == int(c["arg_clearance"][i]), (name, "arg_clearance")
        assert abs(float(got["min_clearance"][j]) - float(c["min_clearance"][i])) <= CLEAR_TOL, (name, "min_clearance")
    return fig


def same_curve(a, ja, b, jb, keys=CURVE + SAMPLE):
    """Curve ja of answer a and curve jb of answer b are equal bit for bit"""
    for k in keys:
        assert np.array_equal(np.asarray(a[k][ja]), np.asarray(b[k][jb])), k


# ---------------------------------------------------------------- the emulator leg
def emu_runner(model, scene):
    """run(...) over ikg_emu_trajectory_check; rc != 0 raises ValueError"""
    import ctypes as C

    import emu as host_emu
    from ikgrasp import _lib
    lib = host_emu.load()
    md, cd = _lib.model_desc(model), _lib.collision_desc(scene)
    nq = model.nq

    def run(points, t_min, t_max, mult, S, cube_fixed, pair_idx, samples_per_wave=0, outputs=None):
        pts = np.ascontiguousarray(points, dtype=np.float64)
        B, n = pts.shape[0], pts.shape[1]
        assert pts.shape[2] == nq
        idx = np.ascontiguousarray(pair_idx, dtype=np.int32).reshape(-1)
        fixed = None if cube_fixed is None else np.ascontiguousarray(cube_fixed, dtype=np.float64).reshape(B, 12)
        res = {k: np.empty(B, dtype=t) for k, t in _lib.TRAJCHECK_CURVE}
        res.update({k: np.empty((B, S) + tail, dtype=t) for k, t, tail in _lib.TRAJCHECK_SAMPLE})
        if outputs is not None:
            res = {k: v for k, v in res.items() if k in outputs}
        out = _lib.TrajCheckOut(*[res[f[0]].ctypes.data if f[0] in res else None
                                  for f in _lib.TRAJCHECK_CURVE + _lib.TRAJCHECK_SAMPLE])
        bset = _lib.BezierSet(pts.ctypes.data, n, float(t_min), float(t_max), float(mult))
        prm = _lib.TrajCheckParams(int(S), _lib.CUBE_CARRIED if fixed is None else _lib.CUBE_FIXED,
                                   int(samples_per_wave))
        rc = lib.ikg_emu_trajectory_check(C.byref(md), C.byref(cd), C.byref(bset), B,
                                          None if fixed is None else fixed.ctypes.data,
                                          idx.ctypes.data if idx.size else None, idx.size, C.byref(prm), C.byref(out))
        if rc != 0:
            raise ValueError(f"ikg_emu_trajectory_check returned {rc}")
        return res

    return run
