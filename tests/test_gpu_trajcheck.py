"""ikg_trajectory_check_batch on the GPU against
tests/golden/trajcheck_cases.npz (tests/golden/make_trajcheck_golden.py; shared
code and the bars in tests/trajcheck_cases.py; the CPU leg on the host emulator
is tests/test_trajcheck.py):

  a. every fixture curve and every output, with host pointers and with device
     tensors: collision flags identical on robust samples, first_collision /
     first_pair / n_collision exact where pinned, grasp / limit / cube within
     16 x the float64 oracle's deviation from 32 digits (floor 1e-12),
     clearance within 1e-7 m where it exceeds 1e-6;
  b. chunking: samples_per_wave 1, 5, S and the launcher's choice give the same
     outputs bit for bit, per sample and per curve;
  c. the composed route on the kernel's own cube output: Solver.collision gives
     the same flag on every sample, Solver.distance the same clearance within
     the bar, and q_k from ikg_bezier_eval_batch reproduces the cube through
     the oracle's FK within the cube bound;
  d. the three-curve neighbour batch and B = 1 give the per-curve results of
     the curves run alone, bit for bit;
  e. control.checktraj on a FittedTrajectories of two fixture paths, and
     path.checkpath on the fixture's polyline;
  f. a generic robot of tests/robot_family.py with its collision scene: the
     device against the host emulator under the same bars;
  g. B = 0 is a no-op.
At most 8 x 33 single-wave checks per call.
"""
import numpy as np
import pytest

import trajcheck_cases as tc

pytestmark = pytest.mark.gpu

NAMES = tc.names()
GROUPS = tc.group_names()


@pytest.fixture(scope="module")
def robot():
    import ikgrasp
    return ikgrasp.setuppinocchio()[0]


def _numpy(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


@pytest.fixture(scope="module")
def run(robot):
    s = robot.solver

    def call(points, t_min, t_max, mult, S, cube_fixed, pair_idx, samples_per_wave=0, device=False):
        cube = "carried" if cube_fixed is None else cube_fixed
        if device:
            import torch
            points = torch.as_tensor(points, device="cuda")
            cube = cube if cube_fixed is None else torch.as_tensor(cube_fixed, device="cuda")
        return _numpy(s.check_curves(points, t_min, t_max, mult=mult, samples=S, cube=cube, pair_idx=pair_idx,
                                     per_sample=True, samples_per_wave=samples_per_wave))

    return call


@pytest.fixture(scope="module")
def answers(run):
    """(a)'s host-pointer answers, computed once: {group index: answer}"""
    c = tc.cases()
    return {g: run(*tc.group_inputs(g), c["pair_idx"]) for g in range(len(GROUPS))}


@pytest.mark.parametrize("name", NAMES)
def test_fixture_curve_host_pointers(answers, name):
    i = tc.index(name)
    g = int(tc.cases()["group"][i])
    tc.compare(i, answers[g], tc.members(g).index(i), verbose=True)
    tc.check_self_fold(answers[g], tc.members(g).index(i))


@pytest.mark.parametrize("group", GROUPS)
def test_fixture_group_device_tensors(run, answers, group):
    g = GROUPS.index(group)
    got = run(*tc.group_inputs(g), tc.cases()["pair_idx"], device=True)
    for j, i in enumerate(tc.members(g)):
        tc.compare(i, got, j)
        tc.same_curve(got, j, answers[g], j)


@pytest.mark.parametrize("group", ["fit", "line", "trio", "fixed"])
def test_chunking_does_not_change_any_output(run, answers, group):
    g = GROUPS.index(group)
    inputs = tc.group_inputs(g)
    S = inputs[4]
    for spw in (1, 5, S):
        got = run(*inputs, tc.cases()["pair_idx"], samples_per_wave=spw)
        for j in range(len(tc.members(g))):
            tc.same_curve(got, j, answers[g], j)


@pytest.mark.parametrize("group", ["fit", "line", "fixed"])
def test_composed_route_agrees(robot, answers, group):
    from oracle import ik_oracle  # noqa: F401  (the oracle FK behind tc.carried_cube)
    c = tc.cases()
    s = robot.solver
    g = GROUPS.index(group)
    pts, t_min, t_max, mult, S, fixed = tc.group_inputs(g)
    times = tc.sample_times(t_min, t_max, S)
    for j, i in enumerate(tc.members(g)):
        q = s.bezier(pts[j], t_min, t_max, mult, times)
        cube = answers[g]["cube"][j]
        assert np.array_equal(s.collision(q, cube), answers[g]["collision"][j].astype(bool)), NAMES[i]
        d = s.distance(q, cube, c["pair_idx"])
        assert np.abs(d - answers[g]["clearance"][j]).max() <= tc.CLEAR_TOL, NAMES[i]
        if fixed is None:
            ref = np.array([tc.cube12(tc.carried_cube(qk)) for qk in q])
            assert np.abs(ref - cube).max() <= tc.bounds()["cube"], NAMES[i]
        else:
            assert all(np.array_equal(row, fixed[j]) for row in cube), NAMES[i]


def test_neighbours_and_single_curves_equal_the_curves_alone(run, answers):
    c = tc.cases()
    for group in ("trio", "fit"):
        g = GROUPS.index(group)
        for j, i in enumerate(tc.members(g)):
            alone = run(*tc.group_inputs(g, [i]), c["pair_idx"])
            tc.same_curve(alone, 0, answers[g], j)
            tc.compare(i, alone, 0)
    g = GROUPS.index("trio")
    order = [2, 0, 1]
    idx = [tc.members(g)[k] for k in order]
    got = run(*tc.group_inputs(g, idx), c["pair_idx"])
    for j, k in enumerate(order):
        tc.same_curve(got, j, answers[g], k)


def test_clearance_is_optional(robot, answers):
    g = GROUPS.index("line")
    pts, t_min, t_max, mult, S, _ = tc.group_inputs(g)
    r = robot.solver.check_curves(pts, t_min, t_max, mult=mult, samples=S, pair_idx=[], per_sample=True)
    for k in ("first_collision", "first_pair", "n_collision", "max_grasp", "arg_grasp", "collision", "grasp", "cube"):
        assert np.array_equal(r[k], answers[g][k]), k
    assert r["min_clearance"][0] == tc.NO_CLEARANCE and r["arg_clearance"][0] == -1
    assert (r["clearance"] == tc.NO_CLEARANCE).all()


def test_checktraj_on_fitted_trajectories(robot):
    """maketraj_batch of the via path and of the straight line qA -> qB: the
    fixture's verdicts for `free` and for `line`"""
    from ikgrasp import control
    c = tc.cases()
    via, qA, qB = c["via"], c["qA"], c["qB"]
    straight = qA + (qB - qA) * np.linspace(0.0, 1.0, 17)[:, None]
    fitted = control.maketraj_batch([qA, qA], [qB, qB], [via, straight], 15.0, solver=robot.solver)
    rep = fitted.check(robot, samples=33, per_sample=True)
    i, k = tc.index("free"), tc.index("line")
    assert rep["ok"].tolist() == [True, False]
    assert rep["first_collision"][0] == c["first_collision"][i] == -1 and rep["max_limit"][0] == 0.0
    assert abs(rep["min_clearance"][0] - c["min_clearance"][i]) <= tc.CLEAR_TOL and rep["arg_clearance"][0] == 32
    assert np.abs(rep["grasp"][0] - tc.samples_of(i, "grasp")).max() <= 1e-6  # the device's fit against fit_oracle's
    assert rep["first_collision"][1] > 0 and rep["first_pair"][1] >= 0 and c["first_collision"][k] > 0
    assert not control.checktraj(robot, fitted, samples=33, min_clearance=0.01)["ok"].any()
    one = control.checktraj(robot, fitted.curves(0), samples=33, per_sample=True)
    for key in tc.CURVE + tc.SAMPLE:
        assert np.array_equal(one[key][0], rep[key][0]), key
    assert control.checktraj(robot, fitted.curves(0)[0], samples=33)["ok"].tolist() == [True]


def test_checkpath_finds_the_connect_jump(robot):
    from ikgrasp import path
    c = tc.cases()
    via, qA, qB = c["via"], c["qA"], c["qB"]
    k = tc.index("line")
    rep = path.checkpath(robot, [via[2], via[1], via[1], qA, qB], per_segment=16)
    assert rep["n_samples"] == 3 * 16 + 1 and not rep["ok"]
    assert rep["segment"] == 2 and rep["first_collision"] == 2 * 16 + int(c["first_collision"][k])
    assert rep["first_pair"] == int(c["first_pair"][k])
    assert rep["n_collision"] == int(c["n_collision"][k])
    assert np.array_equal(rep["collision"][32:], tc.samples_of(k, "collision"))
    free = path.checkpath(robot, [via[2], via[1], qA], per_segment=16)
    assert free["ok"] and free["first_collision"] == -1 and free["n_samples"] == 33


def test_generic_robot_device_equals_emulator():
    """offset_wrist (kSpecGeneric) with its scene: no oracle fixture, the device against the emulator"""
    import robot_family as rf
    from ikgrasp.solver import IKSolver
    m = rf.load_model(rf.COLLISION)
    scene = rf.collision_scene(m)
    qs = np.asarray(rf.q_star(rf.COLLISION), dtype=np.float64)
    z = np.zeros_like(qs)
    pts = np.stack([np.stack([z, (z + qs) / 2, qs]), np.stack([qs, 0.75 * qs, 0.5 * qs]), np.stack([qs, qs * 0.2, -qs])])
    table = len(scene.geoms) - 2
    pair_idx = np.array([k for k, (_, b) in enumerate(scene.pairs) if b == table], dtype=np.int32)
    assert len(pair_idx) > 0
    fixed = np.tile(np.concatenate([np.eye(3).reshape(9), rf.grasp_center(rf.COLLISION)]), (3, 1))
    emu = tc.emu_runner(m, scene)
    s = IKSolver(m, device=0, scene=scene, specialize=False)
    b = tc.bounds()
    for cube in (None, fixed):
        want = emu(pts, 0.0, 2.0, 1.0, 9, cube, pair_idx)
        got = s.check_curves(pts, 0.0, 2.0, samples=9, cube="carried" if cube is None else cube, pair_idx=pair_idx,
                             per_sample=True, samples_per_wave=4)
        assert np.array_equal(got["collision"], want["collision"])
        for k in ("first_collision", "first_pair", "n_collision", "arg_grasp", "arg_limit"):
            assert np.array_equal(got[k], want[k]), k
        for k in ("grasp", "limit", "cube"):
            assert np.abs(got[k] - want[k]).max() <= b[k], (k, float(np.abs(got[k] - want[k]).max()))
        assert np.abs(got["clearance"] - want["clearance"]).max() <= tc.CLEAR_TOL
        for j in range(3):
            tc.check_self_fold(got, j)
    s.close()


def test_zero_curves_is_a_noop(robot):
    r = robot.solver.check_curves(np.zeros((0, 3, 15)), 0.0, 1.0, samples=5, per_sample=True)
    assert all(len(v) == 0 for v in r.values())
    assert r["cube"].shape == (0, 5, 12)
