"""Trajectory check on the CPU (no GPU):

* the fixture tests/golden/trajcheck_cases.npz (answered per sample by the CPU
  oracles, tests/golden/make_trajcheck_golden.py) carries the cases it is
  specified to carry;
* ikg_emu_trajectory_check (csrc/ikg_host_emu.hip: the entry's per-sample
  device functions run serially on the host) against every fixture curve and
  every output, under the fixture's bars: collision flags identical on robust
  samples, first_collision / first_pair / n_collision exact where pinned,
  grasp / limit / cube within 16 x the float64 oracle's own deviation from 32
  digits (floored at 1e-12), clearance within 1e-7 m where it exceeds 1e-6;
* the per-curve outputs are the fold of the per-sample outputs, exactly;
* ikgrasp.path's polyline lift and segment fold, ikgrasp.control's verdict;
* the IKG_EINVAL cases of ikg_trajectory_check_batch that return before any launch.
"""
import ctypes as C

import numpy as np
import pytest

import trajcheck_cases as tc
from ikgrasp import _lib
from ikgrasp.collision import load_nextage_scene
from ikgrasp.control import trajectory_ok
from ikgrasp.model import load_nextage
from ikgrasp.path import fold_segments, polyline_curves


@pytest.fixture(scope="module")
def cases():
    return tc.cases()


@pytest.fixture(scope="module")
def answers(cases):
    """every group through the emulator once: {group index: answer}"""
    # this file's subject is the emulator: a missing build is a failure (emu.load()), not a skip
    run = tc.emu_runner(load_nextage(), load_nextage_scene())
    out = {}
    for g in range(len(tc.group_names())):
        pts, t_min, t_max, mult, S, fixed = tc.group_inputs(g)
        out[g] = run(pts, t_min, t_max, mult, S, fixed, cases["pair_idx"])
    out["run"] = run
    return out


def test_fixture_conditions(cases):
    c = cases
    by = {n: i for i, n in enumerate(tc.names())}
    col = lambda n: tc.samples_of(by[n], "collision")
    assert len(c["names"]) <= 8 and c["group_S"].max() <= 33 and set(c["group_n_points"]) <= {3, 21}
    assert not col("free").any() and (tc.samples_of(by["free"], "clearance") > 0).all()
    i = by["line"]
    assert not col("line")[0] and 0 < c["first_collision"][i] < len(col("line")) - 1
    assert c["pin_pair"][i] and tc.samples_of(i, "hand_cube").any()
    assert [tc.names()[k] for k in tc.members(int(c["group"][by["short"]]))] == ["from0", "short", "last"]
    assert col("from0")[0] and not col("short").any() and col("last").tolist() == [False] * 8 + [True]
    i = by["limit"]
    assert c["max_limit"][i] > 0 and 0 < c["arg_limit"][i] < len(col("limit")) - 1 and not col("limit").any()
    g = tc.samples_of(by["reach"], "grasp")
    assert c["group_fixed"][c["group"][by["reach"]]] and g[-1] < tc.EPSILON < g[0] and (np.diff(g) <= 0).all()
    assert 2 in c["group_S"] and 3 in c["group_n_points"]
    assert c["robust"].mean() >= 0.95
    for i in range(len(c["names"])):
        fc = int(c["first_collision"][i])
        assert fc < 0 or tc.samples_of(i, "robust")[:fc + 1].all()


def test_fixture_pairs_are_the_products_obstacle_pairs(cases):
    assert np.array_equal(cases["pair_idx"], load_nextage_scene().obstacle_pairs())


def test_fixture_times_and_curve_values(cases):
    """the fixture's q rows are the oracle's Horner at the entry's sample times"""
    for i, name in enumerate(tc.names()):
        g = int(cases["group"][i])
        S, t_max = int(cases["group_S"][g]), float(cases["group_t_max"][g])
        t = tc.sample_times(0.0, t_max, S)
        assert t[0] == 0.0 and t[-1] == t_max and len(t) == S
        for k in (0, S // 2, S - 1):
            assert np.array_equal(tc.curve_value(tc.points_of(i), 0.0, t_max, 1.0, t[k]), tc.samples_of(i, "q")[k]), name


@pytest.mark.parametrize("name", ["free", "limit", "line", "from0", "short", "last", "reach", "ends"])
def test_emulator_matches_the_fixture(answers, cases, name):
    i = tc.index(name)
    g = int(cases["group"][i])
    tc.compare(i, answers[g], tc.members(g).index(i), verbose=True)


def test_emulator_per_curve_outputs_are_the_fold_of_its_samples(answers):
    for g in range(len(tc.group_names())):
        for j in range(len(tc.members(g))):
            tc.check_self_fold(answers[g], j)


def test_emulator_first_pair_is_the_lowest_colliding_pair(answers, cases):
    for i, name in enumerate(tc.names()):
        g = int(cases["group"][i])
        fc = int(cases["first_collision"][i])
        if fc >= 0 and cases["pin_pair"][i]:
            assert answers[g]["first_pair"][tc.members(g).index(i)] == tc.samples_of(i, "first_pair_at")[fc], name


def test_emulator_curves_alone_equal_the_batch(answers, cases):
    run = answers["run"]
    g = tc.group_names().index("trio")
    for j, i in enumerate(tc.members(g)):
        pts, t_min, t_max, mult, S, fixed = tc.group_inputs(g, [i])
        tc.same_curve(run(pts, t_min, t_max, mult, S, fixed, cases["pair_idx"]), 0, answers[g], j)


def test_emulator_clearance_is_optional(answers, cases):
    run = answers["run"]
    g = tc.group_names().index("line")
    pts, t_min, t_max, mult, S, fixed = tc.group_inputs(g)
    for r in (run(pts, t_min, t_max, mult, S, fixed, []),
              run(pts, t_min, t_max, mult, S, fixed, cases["pair_idx"],
                  outputs=("first_collision", "first_pair", "n_collision", "max_grasp", "collision"))):
        for k in ("first_collision", "first_pair", "n_collision", "max_grasp", "collision"):
            assert np.array_equal(r[k], answers[g][k]), k
        if "min_clearance" in r:
            assert r["min_clearance"][0] == tc.NO_CLEARANCE and r["arg_clearance"][0] == -1
            assert (r["clearance"] == tc.NO_CLEARANCE).all()


def test_emulator_two_control_points_are_constant(answers, cases):
    """the inherited quirk: a two-point curve is mult * P0 at every time"""
    i = tc.index("line")
    P = tc.points_of(i)[[0, 2]]
    r = answers["run"](P[None], 0.0, 1.0, 1.0, 5, None, cases["pair_idx"])
    assert all(np.array_equal(r["cube"][0][k], r["cube"][0][0]) for k in range(5))
    assert np.abs(r["cube"][0][0] - tc.samples_of(i, "cube")[0]).max() <= tc.bounds()["cube"]


# ---------------------------------------------------------------- the polyline lift (numpy)
def test_polyline_curves_are_the_straight_segments():
    rng = np.random.default_rng(7)
    rows = rng.uniform(-2, 2, (6, 15))
    path = [rows[0], rows[0], rows[1], rows[2], rows[2], rows[2], rows[3], rows[4], rows[5], rows[5]]
    pts, kept = polyline_curves(path)
    assert np.array_equal(kept, rows) and pts.shape == (5, 3, 15)
    for per_segment in (1, 8):
        for i in range(5):
            for k, t in enumerate(tc.sample_times(0.0, 1.0, per_segment + 1)):
                got = tc.curve_value(pts[i], 0.0, 1.0, 1.0, t)
                want = rows[i] + (rows[i + 1] - rows[i]) * t
                assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps * np.abs(rows[i:i + 2]).max()
            assert np.array_equal(tc.curve_value(pts[i], 0.0, 1.0, 1.0, 0.0), rows[i])
            assert np.array_equal(tc.curve_value(pts[i], 0.0, 1.0, 1.0, 1.0), rows[i + 1])
    with pytest.raises(ValueError):
        polyline_curves(np.zeros(15))


def _segment_report(collision, clearance, grasp, limit, first_pair):
    col = np.asarray(collision, dtype=np.uint8)
    n = len(col)
    f = [tc.fold(col[i], None, clearance[i], grasp[i], limit[i]) for i in range(n)]
    rep = {k: np.array([x[k] for x in f]) for k in tc.CURVE if k != "first_pair"}
    rep["first_pair"] = np.asarray(first_pair)
    rep.update(collision=col, clearance=np.asarray(clearance), grasp=np.asarray(grasp), limit=np.asarray(limit))
    return rep


def test_fold_segments_counts_along_the_path():
    # 3 segments of 2 + 1 samples: path samples 0 .. 6; shared ends belong to the later segment
    col = [[0, 0, 1], [0, 1, 0], [0, 0, 1]]  # segment 0's end collides, segment 1's start (the same point) does not
    clearance = [[0.5, 0.4, 0.1], [0.3, 0.2, 0.2], [0.2, 0.6, 0.7]]
    grasp = [[1.0, 2.0, 9.0], [3.0, 3.0, 1.0], [1.0, 0.5, 3.0]]
    limit = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    out = fold_segments(_segment_report(col, clearance, grasp, limit, [40, 41, 42]), 2)
    assert out["n_samples"] == 7
    assert out["collision"].tolist() == [False, False, False, True, False, False, True]
    assert (out["first_collision"], out["segment"], out["first_pair"], out["n_collision"]) == (3, 1, 41, 2)
    assert (out["min_clearance"], out["arg_clearance"]) == (0.2, 3)  # the lowest of the tied samples 3 and 4
    assert (out["max_grasp"], out["arg_grasp"]) == (3.0, 2)  # segment 0's end (9.0) is counted as segment 1's start
    assert (out["max_limit"], out["arg_limit"]) == (0.0, 0)
    # the last segment keeps its own end
    col = [[0, 0, 0], [0, 0, 1]]
    out = fold_segments(_segment_report(col, clearance[:2], grasp[:2], limit[:2], [-1, 17]), 2)
    assert (out["first_collision"], out["segment"], out["first_pair"], out["n_samples"]) == (4, 1, 17, 5)
    col = [[0, 0, 0], [0, 0, 0]]
    out = fold_segments(_segment_report(col, clearance[:2], grasp[:2], limit[:2], [-1, -1]), 2)
    assert (out["first_collision"], out["segment"], out["first_pair"], out["n_collision"]) == (-1, -1, -1, 0)


def test_check_curves_refuses_malformed_inputs_by_name():
    """the argument checks that run before the library is touched"""
    from ikgrasp.solver import IKSolver
    s = IKSolver.__new__(IKSolver)  # no device: only the checks ahead of the call are reached
    s.model, s.scene, s.device = load_nextage(), load_nextage_scene(), 0
    with pytest.raises(ValueError, match="points must be"):
        s.check_curves([[0.0] * 15] * 3, 0.0, 1.0)
    with pytest.raises(ValueError, match="placements"):
        s.check_curves([[[0.0] * 15] * 3] * 2, 0.0, 1.0, cube=np.zeros((3, 12)))
    with pytest.raises(ValueError, match="carried"):
        s.check_curves(np.zeros((1, 3, 15)), 0.0, 1.0, cube="held")
    s.scene = None
    with pytest.raises(RuntimeError, match="scene"):
        s.check_curves(np.zeros((1, 3, 15)), 0.0, 1.0)


def test_launchers_samples_per_wave_rule():
    """the least run that still gives about 2,048 waves, within [1, S]"""
    f = _lib.load().ikg_trajcheck_samples_per_wave
    assert [f(B, 151) for B in (1, 256, 2047, 2048, 4096)] == [1, 19, 76, 151, 151]
    assert f(256, 2) == 1 and f(1 << 40, 33) == 33 and f(0, 151) == 0 and f(4, 1) == 0


def test_trajectory_ok_verdicts():
    rep = {"first_collision": np.array([-1, 3, -1, -1, -1, -1]), "max_limit": np.array([0.0, 0.0, 1e-9, 0.0, 0.0, 0.0]),
           "min_clearance": np.array([0.05, 0.05, 0.05, 0.01, 0.05, tc.NO_CLEARANCE]),
           "arg_clearance": np.array([4, 4, 4, 4, 4, -1]), "max_grasp": np.array([1e-3, 1e-3, 1e-3, 1e-3, 5e-2, 1e-3])}
    assert trajectory_ok(rep).tolist() == [True, False, False, True, True, True]
    assert trajectory_ok(rep, min_clearance=0.02).tolist() == [True, False, False, False, True, True]
    assert trajectory_ok(rep, max_grasp=1e-2).tolist() == [True, False, False, True, False, True]
    assert trajectory_ok(rep, min_clearance=-1.0, max_grasp=1.0).tolist() == [True, False, False, True, True, True]


# ---------------------------------------------------------------- C-ABI refusals before any launch
def test_entry_rejects_bad_arguments_before_touching_the_device(cases):
    lib = _lib.load()
    md = _lib.model_desc(load_nextage())
    h = C.c_void_p()
    assert lib.ikg_model_create(C.byref(md), C.byref(h)) == 0
    HOST = _lib.IKG_FLAG_HOST_POINTERS
    pts = np.ascontiguousarray(tc.points_of(tc.index("line"))[None])
    idx = np.ascontiguousarray(cases["pair_idx"], dtype=np.int32)
    out = _lib.TrajCheckOut()
    p = _lib.trajcheck_params()
    assert (p.samples, p.cube_mode, p.samples_per_wave) == (151, _lib.CUBE_CARRIED, 0)

    def call(bset=None, B=1, fixed=None, pair_idx=idx, n=None, prm=None, o=out, model=h):
        b = bset if bset is not None else _lib.BezierSet(pts.ctypes.data, 3, 0.0, 1.0, 1.0)
        rc = lib.ikg_trajectory_check_batch(model, 0, C.byref(b), B, fixed, None if pair_idx is None else pair_idx.ctypes.data,
                                            len(pair_idx) if n is None else n, C.byref(prm or _lib.trajcheck_params(17)),
                                            C.byref(o), None, HOST)
        return rc, lib.ikg_last_error().decode()

    rc, msg = call()  # no scene attached
    assert rc == -1 and "collision scene" in msg
    assert lib.ikg_model_set_collision(h, C.byref(_lib.collision_desc(load_nextage_scene()))) == 0
    for kw, word in [
        (dict(prm=_lib.trajcheck_params(1)), "samples"),
        (dict(prm=_lib.trajcheck_params(17, 2)), "cube_mode"),
        (dict(prm=_lib.trajcheck_params(17, _lib.CUBE_FIXED)), "cube_fixed"),
        (dict(prm=_lib.trajcheck_params(17, samples_per_wave=-1)), "samples_per_wave"),
        (dict(bset=_lib.BezierSet(pts.ctypes.data, 1, 0.0, 1.0, 1.0)), "2 control points"),
        (dict(bset=_lib.BezierSet(pts.ctypes.data, 65, 0.0, 1.0, 1.0)), "control points"),
        (dict(bset=_lib.BezierSet(pts.ctypes.data, 3, 1.0, 1.0, 1.0)), "t_max"),
        (dict(bset=_lib.BezierSet(None, 3, 0.0, 1.0, 1.0)), "NULL"),
        (dict(pair_idx=np.array([0, len(load_nextage_scene().pairs)], dtype=np.int32)), "pair_idx"),
        (dict(pair_idx=np.array([-1], dtype=np.int32)), "pair_idx"),
        (dict(pair_idx=None, n=3), "pair_idx"),
        (dict(B=-1), "B must"),
    ]:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    bad = pts.copy()
    bad[0, 1, 4] = np.nan
    rc, msg = call(bset=_lib.BezierSet(bad.ctypes.data, 3, 0.0, 1.0, 1.0))
    assert rc == -1 and "not finite" in msg
    fixed = np.full((1, 12), np.inf)
    rc, msg = call(fixed=fixed.ctypes.data, prm=_lib.trajcheck_params(17, _lib.CUBE_FIXED))
    assert rc == -1 and "cube_fixed" in msg
    rc = lib.ikg_trajectory_check_batch(h, 0, None, 1, None, None, 0, C.byref(p), C.byref(out), None, HOST)
    assert rc == -1
    rc = lib.ikg_trajectory_check_batch(h, 0, C.byref(_lib.BezierSet(pts.ctypes.data, 3, 0.0, 1.0, 1.0)), 1, None, None, 0,
                                        None, C.byref(out), None, HOST)
    assert rc == -1 and "params" in lib.ikg_last_error().decode()
    lib.ikg_model_destroy(h)
