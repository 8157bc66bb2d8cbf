"""Trajectory dynamics on the CPU (no GPU):

* ikg_emu_trajectory_dynamics (csrc/ikg_host_emu.hip: the entry's per-sample
  functions run serially on the host) against every case and every output of
  tests/golden/trajdyn_cases.npz (tests/golden/make_trajdyn_golden.py) under
  the fixture's bars: 20 x the float64 oracle's deviation from 50 digits,
  relative to max|out| of the case; args and n_static exact;
* the per-curve outputs are the fold of the per-sample torques, and a batch
  equals its curves run alone;
* ActuatorLimits from the URDF against the committed json, its round trip and
  its refusals; parse_urdf's new fields;
* control.dyntraj / control.retime over a solver whose curve_dynamics is the
  emulator;
* the IKG_EINVAL cases of ikg_trajectory_dynamics_batch that return before any launch.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest

import emu as host_emu
import trajdyn_oracle as to
from ikgrasp import _lib, control
from ikgrasp.model import (ActuatorLimits, load_nextage, load_nextage_actuation, load_nextage_inertia, parse_urdf)

NAMES = ["ref15", "fast", "torque_pos", "torque_neg", "static", "two", "spw5", "trio", "family", "five"]


@pytest.fixture(scope="module")
def runners():
    # this file's subject is the emulator: a missing build is a failure, not a skip
    host_emu.load()
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = to.emu_runner(*to.model_of(model))
        return cache[model]

    return get


@pytest.fixture(scope="module")
def answers(runners):
    """every case through the emulator once"""
    out = {}
    for name in to.names():
        cs = to.case(name)
        out[name] = runners(str(cs["model"]))(*to.inputs(cs), samples_per_wave=int(cs["spw"]))
    return out


def test_fixture_carries_its_cases():
    assert to.names() == NAMES
    c = {n: to.case(n) for n in NAMES}
    assert max(int(x["S"]) for x in c.values()) == 33 and int(c["two"]["S"]) == 2 and int(c["spw5"]["spw"]) == 5
    assert c["five"]["points"].shape[1] == 5 and c["family"]["points"].shape[1:] == (7, 17)
    assert c["ref15"]["range"].tolist() == [0.0, 15.0, 1.0] and c["fast"]["range"][1] == 0.6
    act = load_nextage_actuation()
    assert np.array_equal(c["ref15"]["vlim"], act.velocity) and np.array_equal(c["ref15"]["elim"], act.effort)
    assert c["fast"]["speed_scale"][0] > max(1.0, c["fast"]["torque_scale"][0])
    for n in ("torque_pos", "torque_neg"):
        assert (c[n]["vlim"] == to.NO_LIMIT).all() and c[n]["speed_scale"][0] == 0.0 and c[n]["torque_scale"][0] > 1.0
        assert c[n]["arg_speed"].tolist() == [[0, 0]]  # every entry ties at 0: the lowest sample, the lowest joint
    d = lambda n: (c[n]["tau"] - c[n]["g"])[0][tuple(c[n]["arg_torque_scale"][0])]
    assert d("torque_pos") > 0 > d("torque_neg")
    s = c["static"]
    k, j = s["arg_torque_scale"][0]
    assert s["n_static"][0] > 0 and s["static_use"][0] > 1.0 and abs(s["g"][0, k, j]) < s["elim"][j]
    assert len(c["trio"]["points"]) == 3 and not np.array_equal(c["trio"]["arg_speed"][0], c["trio"]["arg_speed"][1])


@pytest.mark.parametrize("name", NAMES)
def test_emulator_matches_the_fixture(answers, name):
    to.compare(to.case(name), answers[name], verbose=True)


@pytest.mark.parametrize("name", NAMES)
def test_emulator_per_curve_outputs_are_the_fold_of_its_samples(answers, name):
    """the ratios recomputed in numpy from the emulator's own tau and g, and the oracle's v"""
    cs = to.case(name)
    pts, t_min, t_max, mult, S, vlim, elim = to.inputs(cs)
    got = answers[name]
    for b in range(len(pts)):
        _, v, _ = to.curve_states(to.do.F64, pts[b], t_min, t_max, mult, S)
        tau, g = got["tau"][b], got["g"][b]
        efree = elim >= to.NO_LIMIT
        E = np.where(efree, 1.0, elim)
        static = ~efree & (np.abs(g) >= E)
        assert got["n_static"][b] == static.sum()
        use = np.where(efree, 0.0, np.abs(tau) / E)
        assert got["torque_use"][b] == use.max() and tuple(got["arg_torque_use"][b]) == divmod(int(np.argmax(use)), len(E))
        d = tau - g
        with np.errstate(invalid="ignore", divide="ignore"):
            ts = np.where(efree | (d == 0), 0.0, np.sqrt(np.abs(d) / np.where(d > 0, E - g, E + g)))
        ts = np.where(static, -1.0, ts)
        assert abs(got["torque_scale"][b] - ts.max()) <= 4 * np.finfo(np.float64).eps * ts.max()
        assert tuple(got["arg_torque_scale"][b]) == divmod(int(np.argmax(ts)), len(E))
        speed = np.where(vlim >= to.NO_LIMIT, 0.0, np.abs(v) / np.where(vlim >= to.NO_LIMIT, 1.0, vlim))
        assert tuple(got["arg_speed"][b]) == divmod(int(np.argmax(speed)), len(E))


def test_emulator_curves_alone_equal_the_batch(runners, answers):
    cs = to.case("trio")
    run = runners("nextage")
    for j in range(3):
        to.same(run(*to.inputs(cs, [j])), 0, answers["trio"], j)
    got = run(*to.inputs(cs, [2, 0, 1]))
    for j, k in enumerate([2, 0, 1]):
        to.same(got, j, answers["trio"], k)


def test_static_entries_are_counted_and_left_out(runners):
    """one joint that can never hold its gravity torque, the others unlimited: every one of its entries is
    static, and torque_scale is the 0 the unlimited joints contribute, at the first of the tied entries"""
    cs = to.case("ref15")
    pts, t_min, t_max, mult, S, vlim, _ = to.inputs(cs)
    elim = np.full(15, to.NO_LIMIT)
    elim[10] = 1e-3
    r = runners("nextage")(pts, t_min, t_max, mult, S, vlim, elim)
    assert r["n_static"][0] == S and r["torque_scale"][0] == 0.0 and r["arg_torque_scale"].tolist() == [[0, 0]]
    assert r["static_use"][0] == np.abs(r["g"][0][:, 10]).max() / 1e-3 and r["arg_static"][0][1] == 10


# ---------------------------------------------------------------- actuator limits from the URDF
def test_actuator_limits_from_the_urdf_equal_the_committed_json():
    urdf = os.path.join(to.GOLDEN, "NextageaOpen.urdf")
    al = ActuatorLimits.from_urdf(urdf)
    shipped = load_nextage_actuation()
    assert al.velocity.tolist() == [1.0] * 15 and al.effort.tolist() == [100.0] * 3 + [150.0] * 12
    assert np.array_equal(al.velocity, shipped.velocity) and np.array_equal(al.effort, shipped.effort)
    assert ActuatorLimits.from_json(al.to_json()).to_json() == al.to_json()
    tree = parse_urdf(urdf)
    assert [j.velocity for j in tree.joints] == [1.0] * 15 and [j.effort for j in tree.joints][:4] == [100.0] * 3 + [150.0]


def test_actuator_limits_missing_or_zero_are_unlimited():
    xml = """<robot name="r"><link name="a"/><link name="b"/><link name="c"/><link name="d"/>
      <joint name="j0" type="revolute"><parent link="a"/><child link="b"/><axis xyz="0 0 1"/>
        <limit lower="-1" upper="1" velocity="2.5"/></joint>
      <joint name="j1" type="revolute"><parent link="b"/><child link="c"/><axis xyz="0 1 0"/>
        <limit lower="-1" upper="1" effort="0" velocity="0"/></joint>
      <joint name="j2" type="revolute"><parent link="c"/><child link="d"/><axis xyz="1 0 0"/></joint></robot>"""
    al = ActuatorLimits.from_tree(parse_urdf(xml))
    assert al.velocity.tolist() == [2.5, np.inf, np.inf] and al.effort.tolist() == [np.inf] * 3
    text = al.to_json()
    assert "Infinity" not in text and "null" in text
    back = ActuatorLimits.from_json(text)
    assert back.velocity.tolist() == al.velocity.tolist() and back.effort.tolist() == al.effort.tolist()
    for v, e in (([1.0, 0.0], [1.0, 1.0]), ([1.0, 1.0], [-3.0, 1.0]), ([np.nan, 1.0], [1.0, 1.0]), ([1.0], [1.0, 1.0])):
        with pytest.raises(ValueError):
            ActuatorLimits(np.array(v), np.array(e)).validate()
    p = _lib.trajdyn_limits(al.velocity, 3, "velocity")
    assert p.tolist() == [2.5, to.NO_LIMIT, to.NO_LIMIT] and _lib.trajdyn_limits(None, 2, "x").tolist() == [to.NO_LIMIT] * 2
    assert _lib.trajdyn_limits(4.0, 2, "x").tolist() == [4.0, 4.0]
    with pytest.raises(ValueError):
        _lib.trajdyn_limits([1.0, np.nan], 2, "effort")


def test_the_robot_carries_the_limits():
    from ikgrasp.scene import Robot
    act = Robot().actuation
    assert act.velocity.tolist() == [1.0] * 15 and act.effort.tolist() == [100.0] * 3 + [150.0] * 12


# ---------------------------------------------------------------- dyntraj / retime over the emulator
class _EmuSolver:
    """IKSolver.curve_dynamics answered by the host emulator"""

    def __init__(self, run, nq):
        self.run, self.nq = run, nq

    def curve_dynamics(self, points, t_min, t_max, mult=1.0, samples=151, velocity=None, effort=None,
                       per_sample=False, samples_per_wave=0):
        r = self.run(points, t_min, t_max, mult, samples, _lib.trajdyn_limits(velocity, self.nq, "velocity"),
                     _lib.trajdyn_limits(effort, self.nq, "effort"), samples_per_wave)
        return r if per_sample else {k: v for k, v in r.items() if k not in to.SAMPLE}


@pytest.fixture(scope="module")
def robot(runners):
    return types.SimpleNamespace(solver=_EmuSolver(runners("nextage"), 15), actuation=load_nextage_actuation())


def test_dyntraj_verdict_and_least_duration(robot, answers):
    P = to.case("ref15")["points"][0]
    slow, fast = control.Curve(list(P), 0.0, 15.0), control.Curve(list(P), 0.0, 0.6)
    rep = control.dyntraj(robot, slow, samples=33, per_sample=True)
    to.same(rep, 0, answers["ref15"], 0)
    assert rep["ok"].tolist() == [True]
    assert rep["least_duration"][0] == 15.0 * max(rep["speed_scale"][0], rep["torque_scale"][0])
    rep = control.dyntraj(robot, (fast, None, None), samples=33)
    to.same(rep, 0, answers["fast"], 0, keys=to.CURVE_KEYS)
    assert rep["ok"].tolist() == [False] and "tau" not in rep
    assert rep["least_duration"][0] == 0.6 * rep["speed_scale"][0]
    e = load_nextage_actuation().effort.copy()
    e[10] = 8.0
    rep = control.dyntraj(robot, slow, samples=33, effort=e)
    assert rep["n_static"][0] == to.case("static")["n_static"][0] and not rep["ok"][0] and np.isinf(rep["least_duration"][0])
    with pytest.raises(ValueError, match="n_static"):
        control.retime(robot, slow, samples=33, effort=e)
    free = control.dyntraj(types.SimpleNamespace(solver=robot.solver), fast, samples=33)  # a robot without limits
    assert free["ok"].tolist() == [True] and free["least_duration"][0] == 0.0 and free["static_use"][0] == 0.0


def test_retime_one_trajectory(robot):
    P = to.case("ref15")["points"][0]
    fast = control.Curve(list(P), 0.0, 0.6)
    before = control.dyntraj(robot, fast, samples=33)
    q, v, a = control.retime(robot, (fast, fast.derivative(1), fast.derivative(2)), samples=33)
    assert q.T_min_ == 0.0 and q.T_max_ == before["least_duration"][0] and q.mult_T_ == 1.0
    assert all(np.array_equal(x, y) for x, y in zip(q.control_points_, fast.control_points_))
    assert v.mult_T_ == 1.0 * (1.0 / q.T_max_) and a.mult_T_ == v.mult_T_ * (1.0 / q.T_max_)
    assert len(v.control_points_) == 15 and len(a.control_points_) == 14 and v.T_max_ == a.T_max_ == q.T_max_
    after = control.dyntraj(robot, q, samples=33)
    # the scaling law: at the least duration the binding ratio is 1; v scales as 1 / s exactly, and each of the
    # two evaluations is within the fixture's bar of its own truth
    cs = to.case("fast")
    assert abs(max(after["speed_scale"][0], after["torque_scale"][0]) - 1.0) <= 2 * to.bar(cs, "speed_scale") / cs["speed_scale"][0]
    assert after["torque_use"][0] < 1.0 and after["n_static"][0] == 0
    wide = control.retime(robot, fast, margin=1.25, samples=33)[0]
    assert wide.T_max_ == 1.25 * before["least_duration"][0]
    assert control.dyntraj(robot, wide, samples=33)["ok"].tolist() == [True]


def test_retime_a_batch(robot):
    pts = to.case("trio")["points"]
    fitted = control.FittedTrajectories(pts, None, None, np.zeros(3), 3.0)
    rep = fitted.dynamics(robot, samples=17)
    to.same(rep, 1, control.dyntraj(robot, control.Curve(list(pts[1]), 0.0, 3.0), samples=17), 0, keys=to.CURVE_KEYS)
    durations, again = control.retime(robot, fitted, samples=17)
    assert np.array_equal(durations, rep["least_duration"]) and again.t_max == durations.max() and again.t_min == 0.0
    assert again.points is fitted.points
    assert again.dynamics(robot, samples=17)["ok"].sum() >= 2  # the binding curve sits at 1 up to rounding
    _, padded = control.retime(robot, fitted, margin=1.01, samples=17)
    assert padded.dynamics(robot, samples=17)["ok"].all()


def test_curve_dynamics_refuses_malformed_points_by_name():
    from ikgrasp.solver import IKSolver
    s = IKSolver.__new__(IKSolver)  # no device: only the checks ahead of the call are reached
    s.model, s.device = load_nextage(), 0
    with pytest.raises(ValueError, match="points must be"):
        s.curve_dynamics([[0.0] * 15] * 5, 0.0, 1.0)
    with pytest.raises(ValueError, match="points must be"):
        s.curve_dynamics(np.zeros((1, 5, 14)), 0.0, 1.0)


# ---------------------------------------------------------------- C-ABI refusals before any launch
def test_entry_rejects_bad_arguments_before_touching_the_device(runners):
    lib = _lib.load()
    md = _lib.model_desc(load_nextage())
    h = C.c_void_p()
    assert lib.ikg_model_create(C.byref(md), C.byref(h)) == 0
    HOST = _lib.IKG_FLAG_HOST_POINTERS
    pts = np.ascontiguousarray(to.case("five")["points"])
    out = _lib.TrajDynOut()
    p = _lib.TrajDynParams()
    lib.ikg_trajdyn_params_default(C.byref(p))
    assert (p.samples, p.samples_per_wave) == (151, 0)
    assert list(p.velocity_limit) == [to.NO_LIMIT] * 32 and list(p.effort_limit) == [to.NO_LIMIT] * 32

    def call(bset=None, B=1, prm=None, o=out, flags=HOST):
        b = bset if bset is not None else _lib.BezierSet(pts.ctypes.data, 5, 0.0, 1.0, 1.0)
        rc = lib.ikg_trajectory_dynamics_batch(h, 0, C.byref(b), B, C.byref(prm or _lib.trajdyn_params(15, 9)),
                                               C.byref(o), None, flags)
        return rc, lib.ikg_last_error().decode()

    rc, msg = call()  # no inertias attached
    assert rc == -1 and "inertia" in msg
    assert lib.ikg_model_set_inertia(h, C.byref(_lib.inertia_desc(load_nextage_inertia()))) == 0

    def limits(which, j, x):
        prm = _lib.trajdyn_params(15, 9)
        getattr(prm, which)[j] = x
        return prm

    long = np.zeros((1, 65, 15))
    for kw, word in [
        (dict(prm=_lib.trajdyn_params(15, 1)), "samples"),
        (dict(prm=_lib.trajdyn_params(15, 9, samples_per_wave=-1)), "samples_per_wave"),
        (dict(prm=limits("velocity_limit", 3, 0.0)), "velocity_limit[3]"),
        (dict(prm=limits("velocity_limit", 14, -1.0)), "velocity_limit[14]"),
        (dict(prm=limits("effort_limit", 0, 0.0)), "effort_limit[0]"),
        (dict(prm=limits("effort_limit", 7, float("nan"))), "effort_limit[7]"),
        (dict(prm=limits("effort_limit", 7, float("inf"))), "effort_limit[7]"),
        (dict(bset=_lib.BezierSet(pts.ctypes.data, 4, 0.0, 1.0, 1.0)), "at least 5"),
        (dict(bset=_lib.BezierSet(pts.ctypes.data, 2, 0.0, 1.0, 1.0)), "at least 5"),
        (dict(bset=_lib.BezierSet(long.ctypes.data, 65, 0.0, 1.0, 1.0)), "control points"),
        (dict(bset=_lib.BezierSet(pts.ctypes.data, 5, 1.0, 1.0, 1.0)), "t_max"),
        (dict(bset=_lib.BezierSet(pts.ctypes.data, 5, 2.0, 1.0, 1.0)), "t_max"),
        (dict(bset=_lib.BezierSet(None, 5, 0.0, 1.0, 1.0)), "NULL"),
        (dict(B=-1), "B must"),
    ]:
        for flags in (HOST, 0):  # the limits are checked with device pointers too
            rc, msg = call(flags=flags, **kw)
            assert rc == -1 and word in msg, (kw, flags, rc, msg)
    bad = pts.copy()
    bad[0, 2, 4] = np.nan
    rc, msg = call(bset=_lib.BezierSet(bad.ctypes.data, 5, 0.0, 1.0, 1.0))
    assert rc == -1 and "not finite" in msg
    bad[0, 2, 4] = np.inf
    assert call(bset=_lib.BezierSet(bad.ctypes.data, 5, 0.0, 1.0, 1.0))[0] == -1
    rc = lib.ikg_trajectory_dynamics_batch(h, 0, None, 1, C.byref(p), C.byref(out), None, HOST)
    assert rc == -1
    b = _lib.BezierSet(pts.ctypes.data, 5, 0.0, 1.0, 1.0)
    assert lib.ikg_trajectory_dynamics_batch(h, 0, C.byref(b), 1, None, C.byref(out), None, HOST) == -1
    assert "params" in lib.ikg_last_error().decode()
    assert lib.ikg_trajectory_dynamics_batch(h, 0, C.byref(b), 1, C.byref(p), None, None, HOST) == -1
    assert "out" in lib.ikg_last_error().decode()
    assert lib.ikg_trajectory_dynamics_batch(None, 0, C.byref(b), 1, C.byref(p), C.byref(out), None, HOST) == -1
    lib.ikg_model_destroy(h)
    # the emulator refuses the same limits
    run = runners("nextage")
    V, E = np.full(15, 1.0), np.full(15, 100.0)
    for args in ((pts, 0.0, 1.0, 1.0, 1, V, E), (pts[:, :4], 0.0, 1.0, 1.0, 9, V, E), (pts, 1.0, 1.0, 1.0, 9, V, E),
                 (pts, 0.0, 1.0, 1.0, 9, V * 0.0, E), (pts, 0.0, 1.0, 1.0, 9, V, -E)):
        with pytest.raises(ValueError):
            run(*args)
