"""ikg_trajectory_dynamics_batch on the GPU against
tests/golden/trajdyn_cases.npz (tests/golden/make_trajdyn_golden.py; the
definitions, the bars and the shared code in tests/trajdyn_oracle.py; the CPU
leg on the host emulator is tests/test_trajdyn.py):

  a. every case and every output with host pointers and with device tensors:
     tau, g and the ratios within 20 x the float64 oracle's deviation from 50
     digits (relative to max|out| of the case), args and n_static exact;
  b. chunking: samples_per_wave 1, 5, S and the launcher's choice give every
     output bit for bit;
  c. the three-curve batch equals its curves run alone, bit for bit;
  d. the composed route: Solver.bezier for q, v, a, then Solver.dynamics with
     M @ a + nle, agrees with tau within the sum of the two bars (this entry's
     and the dynamics kernel's 1e-12 max(1, max|.|) of tests/test_gpu_dynamics.py
     carried through the product), and its g with g;
  e. the scaling law: torque_pos / torque_neg again at t_max' = t_min + s T give
     max(speed_scale, torque_scale) = 1 within the fixture's bar;
  f. control.dyntraj and control.retime on a two-path FittedTrajectories;
  g. the family robot mixed_17 (32 lanes per sample): device against emulator;
  h. B = 0 is a no-op.
At most 3 x 33 samples per call.
"""
import numpy as np
import pytest

import trajdyn_oracle as to

pytestmark = pytest.mark.gpu

NAMES = to.names()
DYN_BAR = 1e-12  # tests/test_gpu_dynamics.py: the dynamics kernel's fp64 M / nle / g within 1e-12 max(1, max|ref|)


@pytest.fixture(scope="module")
def robot():
    import ikgrasp
    return ikgrasp.setuppinocchio()[0]


@pytest.fixture(scope="module")
def solvers(robot):
    """{model name: IKSolver}; the family robot's is built here with its seeded inertias"""
    from ikgrasp.solver import IKSolver
    m, bi = to.model_of("mixed_17")
    fam = IKSolver(m, device=0, specialize=False)
    fam.set_inertia(bi)
    yield {"nextage": robot.solver, "mixed_17": fam}
    fam.close()


def _numpy(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


@pytest.fixture(scope="module")
def run(solvers):
    def call(cs, idx=None, samples_per_wave=None, device=False, t_max=None):
        pts, t_min, t1, mult, S, vlim, elim = to.inputs(cs, idx)
        if device:
            import torch
            pts = torch.as_tensor(pts, device="cuda")
        spw = int(cs["spw"]) if samples_per_wave is None else samples_per_wave
        return _numpy(solvers[str(cs["model"])].curve_dynamics(
            pts, t_min, t1 if t_max is None else t_max, mult=mult, samples=S, velocity=vlim, effort=elim,
            per_sample=True, samples_per_wave=spw))

    return call


@pytest.fixture(scope="module")
def answers(run):
    """(a)'s host-pointer answers, computed once"""
    return {name: run(to.case(name)) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_fixture_case_host_pointers(answers, name):
    to.compare(to.case(name), answers[name], verbose=True)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_case_device_tensors(run, answers, name):
    cs = to.case(name)
    got = run(cs, device=True)
    to.compare(cs, got)
    for j in range(len(cs["points"])):
        to.same(got, j, answers[name], j)


@pytest.mark.parametrize("name", ["ref15", "static", "two", "spw5", "trio", "family", "five"])
def test_chunking_does_not_change_any_output(run, answers, name):
    cs = to.case(name)
    for spw in (1, 5, int(cs["S"]), 0):
        got = run(cs, samples_per_wave=spw)
        for j in range(len(cs["points"])):
            to.same(got, j, answers[name], j)


def test_batch_equals_its_curves_alone(run, answers):
    cs = to.case("trio")
    for j in range(3):
        alone = run(cs, idx=[j])
        to.same(alone, 0, answers["trio"], j)
        to.compare(cs, alone, rows=[j])
    got = run(cs, idx=[2, 0, 1])
    for j, k in enumerate([2, 0, 1]):
        to.same(got, j, answers["trio"], k)


@pytest.mark.parametrize("name", ["ref15", "fast", "trio", "family"])
def test_composed_route_agrees(solvers, answers, name):
    from ikgrasp.control import Curve
    cs = to.case(name)
    s = solvers[str(cs["model"])]
    pts, t_min, t_max, mult, S, _, _ = to.inputs(cs)
    times = np.array(to.sample_times(t_min, t_max, S))
    for b in range(len(pts)):
        c = Curve(list(pts[b]), t_min, t_max, mult)
        q, v, a = (s.bezier(np.array(x.control_points_), x.T_min_, x.T_max_, x.mult_T_, times)
                   for x in (c, c.derivative(1), c.derivative(2)))
        r = s.dynamics(q, v, outputs=("M", "nle", "g"))
        tau = np.einsum("kij,kj->ki", r["M"], a) + r["nle"]
        # |dM a + dnle| <= bar(M) sum_j |a_j| + bar(nle), then this entry's own bar
        composed = DYN_BAR * max(1.0, np.abs(r["M"]).max()) * np.abs(a).sum(axis=1).max() \
            + DYN_BAR * max(1.0, np.abs(r["nle"]).max())
        err = np.abs(tau - answers[name]["tau"][b]).max()
        errg = np.abs(r["g"] - answers[name]["g"][b]).max()
        print(name, b, f"tau {err:.2e} (bars {composed:.2e} + {to.bar(cs, 'tau'):.2e}), g {errg:.2e}")
        assert err <= composed + to.bar(cs, "tau"), (name, b, err)
        assert errg <= DYN_BAR * max(1.0, np.abs(r["g"]).max()) + to.bar(cs, "g"), (name, b, errg)


@pytest.mark.parametrize("name", ["torque_pos", "torque_neg"])
def test_scaling_law(run, answers, name):
    cs = to.case(name)
    got = run(cs, t_max=float(cs["t_max_scaled"]))
    scale = max(got["speed_scale"][0], got["torque_scale"][0])
    print(name, f"scale at t_max' {scale!r}: off 1 by {abs(scale - 1.0):.2e} (bar {to.BAR_FACTOR * float(cs['scale_dev']):.2e})")
    assert abs(scale - 1.0) <= to.BAR_FACTOR * float(cs["scale_dev"])
    assert np.array_equal(got["arg_torque_scale"], answers[name]["arg_torque_scale"]) and got["n_static"][0] == 0


def test_dyntraj_and_retime_on_fitted_trajectories(robot):
    """maketraj_batch of the trajectory check's via path and of the straight line between its two grasps"""
    import trajcheck_cases as tc
    from ikgrasp import control
    c = tc.cases()
    via, qA, qB = c["via"], c["qA"], c["qB"]
    straight = qA + (qB - qA) * np.linspace(0.0, 1.0, 17)[:, None]
    fitted = control.maketraj_batch([qA, qA], [qB, qB], [via, straight], 15.0, solver=robot.solver)
    rep = fitted.dynamics(robot, samples=33, per_sample=True)
    assert rep["tau"].shape == (2, 33, 15) and rep["arg_speed"].shape == (2, 2)
    assert (rep["n_static"] == 0).all() and (rep["least_duration"] > 0).all()
    T = 15.0
    assert np.array_equal(rep["least_duration"], T * np.maximum(rep["speed_scale"], rep["torque_scale"]))
    assert np.array_equal(rep["ok"], (rep["speed_scale"] <= 1) & (rep["torque_use"] <= 1))
    one = control.dyntraj(robot, fitted.curves(1), samples=33, per_sample=True)
    to.same(one, 0, rep, 1)
    durations, again = control.retime(robot, fitted, margin=1.01, samples=33)
    assert np.array_equal(durations, 1.01 * rep["least_duration"]) and again.t_max == durations.max()
    assert again.dynamics(robot, samples=33)["ok"].all()
    q, v, a = control.retime(robot, fitted.curves(0), margin=1.01, samples=33)
    assert q.T_max_ == durations[0] and v.mult_T_ == 1.0 / q.T_max_ and len(a.control_points_) == 19
    tight = control.dyntraj(robot, q, samples=33)
    assert tight["ok"].tolist() == [True]
    # 1.01 T_least: the binding ratio is 1 / 1.01 (speed) or 1 / 1.01^2 (torque) up to rounding
    assert 0.98 <= max(tight["speed_scale"][0], tight["torque_scale"][0]) < 1.0
    short = control.retime(robot, fitted.curves(0), margin=0.5, samples=33)[0]
    assert not control.dyntraj(robot, short, samples=33)["ok"][0]


def test_family_robot_device_equals_emulator(run, answers):
    cs = to.case("family")
    emu = to.emu_runner(*to.model_of("mixed_17"))
    want = emu(*to.inputs(cs))
    got = answers["family"]
    for k in to.SAMPLE + to.RATIOS:
        assert np.abs(got[k] - want[k]).max() <= 2 * to.bar(cs, k), (k, float(np.abs(got[k] - want[k]).max()))
    for k in tuple(to.ARGS.values()) + ("n_static",):
        assert np.array_equal(got[k], want[k]), k


def test_zero_curves_is_a_noop(robot):
    r = robot.solver.curve_dynamics(np.zeros((0, 5, 15)), 0.0, 1.0, samples=5, per_sample=True)
    assert all(len(v) == 0 for v in r.values())
    assert r["tau"].shape == (0, 5, 15) and r["arg_speed"].shape == (0, 2)
