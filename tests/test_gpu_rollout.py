"""Forward dynamics, Bezier desired state and the closed-loop rollout on the GPU
(ikg_forward_dynamics_batch, ikg_bezier_eval_batch, ikg_control_rollout)
against tests/golden/rollout_cases.npz (make_rollout_golden.py).

Bounds: the Bezier values 4 n 2^-52 max|P| |mult|; forward dynamics tol_fd and
the rollouts' per-tick tol_q / tol_v / tol_tau as stored in the fixture (20 x
the float64 restatement's error against the 50-digit evaluation, relative to
max|output|).  Everything else here is bit-equality between calls."""
import ctypes as C
import os

import numpy as np
import pytest

import rollout_cases as rc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FINAL = ("q", "v", "t")
ALL = FINAL + rc.HIST


@pytest.fixture(scope="module")
def d():
    return rc.load()


@pytest.fixture(scope="module")
def dc():
    return dict(np.load(os.path.join(GOLDEN, "dynamics_cases.npz")))


@pytest.fixture(scope="module")
def nextage_rollouts(solver, d):
    """The fixture's 16 starts x 32 ticks, run once (eight calls: one per curve pair and gain set)."""
    return rc.run_rollouts(solver, d, "nextage", 32)


@pytest.fixture(scope="module")
def one_call(solver, d):
    """All 16 starts under ONE curve pair and the default gains, 8 ticks: what
    the batch-shape, composition and pointer tests compare against."""
    trajs = rc.traj_curves(d, 1, False)
    r = solver.rollout(d["ro_q0"], d["ro_v0"], trajs, t0=d["ro_t0"], ticks=8, record_every=1, outputs=ALL)
    return trajs, r


def _other_solver(name):
    from ikgrasp.solver import IKSolver
    m, bi = rc.models()[name]
    return IKSolver(m, device=0, specialize=False), bi


# ---------------------------------------------------------------- against the fixture
def test_bezier_matches_fixture(solver, d):
    rc.check_bezier(solver, d)
    P = np.array([[1.0, -2.0, 0.5], [7.0, 7.0, 7.0]])
    assert np.array_equal(solver.bezier(P, 1.0, 3.0, 0.25, [1.0, 2.0, 3.0]), np.tile(0.25 * P[0], (3, 1)))
    from ikgrasp import _lib
    with pytest.raises(_lib.IkgError):
        solver.bezier(np.vstack([P, P[:1]]), 1.0, 3.0, 1.0, [3.5])


def test_forward_dynamics_within_measured_bound(solver, d, dc):
    """Bound: tol_fd = 4.68e-14 of max|qdd| (M about each joint's own origin; tests/test_rollout.py)."""
    rc.check_forward_dynamics(solver, dc["q"], dc["v"], dc["tau"], d["fd_qdd_mp"], float(d["tol_fd"]), "nextage")


def test_forward_dynamics_satisfies_its_equation(solver, d, dc):
    rc.check_forward_dynamics_equation(solver, dc["q"], dc["v"], dc["tau"], float(d["tol_fd"]), "nextage")


def test_forward_dynamics_of_the_32_joint_model(d):
    """16 states of mixed_axes (nq = 32, the G = 32 instantiation).  Bound:
    mixed_tol_fd = 1.46e-14 of max|qdd| (20 x a float64 error of 7.3e-16)."""
    s, bi = _other_solver("mixed")
    try:
        s.set_inertia(bi)
        a = (s, d["mixed_fd_q"], d["mixed_fd_v"], d["mixed_fd_tau"])
        rc.check_forward_dynamics_equation(*a, float(d["mixed_tol_fd"]), "mixed_axes")
        rc.check_forward_dynamics(*a, d["mixed_fd_qdd_mp"], float(d["mixed_tol_fd"]), "mixed_axes")
    finally:
        s.close()


def test_rollouts_within_per_tick_bounds(nextage_rollouts, d):
    rc.check_rollouts(nextage_rollouts, d, "nextage", "gpu")


@pytest.mark.parametrize("name,ticks", [("tilted", 16), ("mixed", 8)])
def test_other_models_within_per_tick_bounds(d, name, ticks):
    s, bi = _other_solver(name)
    try:
        with pytest.raises(Exception, match="inertia"):  # an explicit model comes without inertias
            s.rollout(d[name + "_q0"], d[name + "_v0"], rc.groups(d, name)[0][1], ticks=1)
        s.set_inertia(bi)
        got = rc.run_rollouts(s, d, name, ticks)
    finally:
        s.close()
    rc.check_rollouts(got, d, name, "gpu")


def test_first_torque_is_control_torques(solver, d, nextage_rollouts):
    """tau_hist[:, 0] is the torque law at the start state and the desired state at t0."""
    worst, equal = 0.0, True
    for rows, (cq, cv), gains in rc.groups(d, "nextage"):
        t0 = d["ro_t0"][rows]
        q_des = np.vstack([solver.bezier(*cq, [t]) for t in t0])
        v_des = np.vstack([solver.bezier(*cv, [t]) for t in t0])
        tau = solver.control_torques(d["ro_q0"][rows], d["ro_v0"][rows], q_des, v_des, outputs=("tau",), **gains)["tau"]
        got = nextage_rollouts["tau"][rows, 0]
        worst = max(worst, np.abs(got - tau).max() / np.abs(d["ro_tau_mp"]).max())
        equal = equal and np.array_equal(got, tau)
    print(f"tau_hist[:, 0] vs control_torques: {worst:.3e} of max|tau| (bound {d['tol_tau'][0]:.3e}); bit-equal: {equal}")
    assert worst <= d["tol_tau"][0]
    assert equal  # the solve kernel and the step kernel run the same phases on the same scratch


# ---------------------------------------------------------------- one call against another, bit for bit
@pytest.mark.parametrize("B", [1, 3, 4, 5, 33])
def test_batch_shapes(solver, d, one_call, B):
    """4 states per wave with tails, and more than one workgroup: row i of a
    B-row call equals row i % 16 of the 16-row call."""
    trajs, ref = one_call
    idx = np.arange(B) % 16
    r = solver.rollout(d["ro_q0"][idx], d["ro_v0"][idx], trajs, t0=d["ro_t0"][idx], ticks=8, record_every=1, outputs=ALL)
    for k in ALL:
        assert np.array_equal(r[k], ref[k][idx]), k


def test_two_states_per_wave_batch_shapes(d):
    """The G = 32 instantiation (nq = 32, 2 states per wave): B = 1, 3 against B = 2."""
    s, bi = _other_solver("mixed")
    try:
        s.set_inertia(bi)
        _, trajs, _ = rc.groups(d, "mixed")[0]
        run = lambda idx: s.rollout(d["mixed_q0"][idx], d["mixed_v0"][idx], trajs, t0=d["mixed_t0"][idx], ticks=4,
                                    record_every=1, outputs=ALL)
        ref = run(np.arange(2))
        for B in (1, 3):
            idx = np.arange(B) % 2
            r = run(idx)
            for k in ALL:
                assert np.array_equal(r[k], ref[k][idx]), (B, k)
    finally:
        s.close()


def test_composition(solver, d, one_call):
    """One call of 8 ticks equals 8 calls of 1 tick fed with the returned q, v, t."""
    trajs, ref = one_call
    q, v, t = d["ro_q0"], d["ro_v0"], d["ro_t0"]
    for k in range(8):
        r = solver.rollout(q, v, trajs, t0=t, ticks=1, record_every=1, outputs=ALL)
        q, v, t = r["q"], r["v"], r["t"]
        for name in rc.HIST:
            assert np.array_equal(r[name][:, 0], ref[name][:, k]), (name, k)
    for name, x in (("q", q), ("v", v), ("t", t)):
        assert np.array_equal(x, ref[name]), name


def test_record_every_and_untouched_inputs(solver, d, one_call):
    trajs, ref = one_call
    q0, v0, t0 = d["ro_q0"].copy(), d["ro_v0"].copy(), d["ro_t0"].copy()
    r = solver.rollout(q0, v0, trajs, t0=t0, ticks=8, record_every=4, outputs=ALL)
    for k in rc.HIST:
        assert r[k].shape == (16, 2, 15) and np.array_equal(r[k], ref[k][:, 3::4]), k
    f = solver.rollout(q0, v0, trajs, t0=t0, ticks=8)  # no history, state rows in the outputs
    h = solver.rollout(q0, v0, trajs, t0=t0, ticks=8, record_every=1, outputs=rc.HIST)  # state rows in scratch
    for k in FINAL:
        assert np.array_equal(r[k], ref[k]) and np.array_equal(f[k], ref[k]), k
    for k in rc.HIST:
        assert np.array_equal(h[k], ref[k]), k
    assert np.array_equal(q0, d["ro_q0"]) and np.array_equal(v0, d["ro_v0"]) and np.array_equal(t0, d["ro_t0"])
    z = solver.rollout(q0, v0, trajs, ticks=0)
    assert np.array_equal(z["q"], q0) and np.array_equal(z["v"], v0) and np.all(z["t"] == trajs[0][1])


def test_across_scratch_chunks(solver, d):
    """More states than one pass of the scratch holds (65,536), 2 ticks, no
    history: every row equals the B = 97 call's row of the same start."""
    trajs = rc.traj_curves(d, 1, False)
    i97 = np.arange(97) % 16
    ref = solver.rollout(d["ro_q0"][i97], d["ro_v0"][i97], trajs, t0=d["ro_t0"][i97], ticks=2)
    idx = np.arange(65536 + 97) % 97
    r = solver.rollout(d["ro_q0"][i97][idx], d["ro_v0"][i97][idx], trajs, t0=d["ro_t0"][i97][idx], ticks=2)
    for k in FINAL:
        assert np.array_equal(r[k], ref[k][idx]), k


def test_host_and_device_calls_agree(solver, d, dc, one_call):
    import torch
    trajs, ref = one_call
    dev = lambda x: torch.tensor(x, device="cuda", dtype=torch.float64)
    q0, v0, t0 = dev(d["ro_q0"]), dev(d["ro_v0"]), dev(d["ro_t0"])
    r = solver.rollout(q0, v0, trajs, t0=t0, ticks=8, record_every=1, outputs=ALL)
    fd = solver.forward_dynamics(dev(dc["q"]), dev(dc["v"]), dev(dc["tau"]))
    bz = solver.bezier(*trajs[0], dev(d["bez_times"]))
    torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(r[k].cpu().numpy(), ref[k]), k
    assert np.array_equal(q0.cpu().numpy(), d["ro_q0"]) and np.array_equal(t0.cpu().numpy(), d["ro_t0"])
    assert np.array_equal(fd.cpu().numpy(), solver.forward_dynamics(dc["q"], dc["v"], dc["tau"]))
    assert np.array_equal(bz.cpu().numpy(), solver.bezier(*trajs[0], d["bez_times"]))


def test_capture_and_replay_on_a_side_stream(solver, d, one_call):
    import torch
    trajs, ref = one_call
    idx = np.arange(33) % 16
    dev = lambda x: torch.tensor(x[idx], device="cuda", dtype=torch.float64)
    q0, v0, t0 = dev(d["ro_q0"]), dev(d["ro_v0"]), dev(d["ro_t0"])
    run = lambda: solver.rollout(q0, v0, trajs, t0=t0, ticks=8, record_every=1, outputs=ALL)
    direct = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up off the default stream, as torch recommends before capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captures on a side stream, which is the current stream inside
        cap = run()
    for k in ALL:
        cap[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(cap[k].cpu().numpy(), direct[k].cpu().numpy()), k
        assert np.array_equal(cap[k].cpu().numpy(), ref[k][idx]), k
    del graph


def test_empty_batch_touches_nothing(solver, d):
    from ikgrasp import _lib
    trajs = rc.traj_curves(d, 1, False)
    r = solver.rollout(np.zeros((0, 15)), np.zeros((0, 15)), trajs, ticks=4, record_every=2, outputs=ALL)
    assert r["q"].shape == (0, 15) and r["q_hist"].shape == (0, 2, 15) and r["t"].shape == (0,)
    assert solver.forward_dynamics(np.zeros((0, 15)), None, np.zeros((0, 15))).shape == (0, 15)
    guard = np.full(15, 7.0)
    p = guard.ctypes.data
    bq, _keep = _lib.bezier_desc(trajs[0], 15)
    prm = _lib.rollout_params(4, record_every=1)
    out = _lib.RolloutOut(p, p, p, p, p, p)
    HOST = _lib.IKG_FLAG_HOST_POINTERS
    assert solver.lib.ikg_control_rollout(solver._h, 0, p, p, p, 0, C.byref(bq), C.byref(bq), C.byref(prm),
                                          C.byref(out), None, HOST) == 0
    assert solver.lib.ikg_forward_dynamics_batch(solver._h, 0, p, p, p, 0, p, None, HOST) == 0
    assert solver.lib.ikg_bezier_eval_batch(0, trajs[0][0].ctypes.data, len(trajs[0][0]), 15, 0.0, 15.0, 1.0, p, 0, p,
                                            None, HOST) == 0
    assert np.all(guard == 7.0)


def test_simulation_loop_agrees_with_rollout(d, nextage_rollouts):
    """The reference's loop with `ikgrasp.control.Simulation` and `controllaw`, 4 ticks."""
    import ikgrasp
    from ikgrasp import control
    robot, _, _, cube = ikgrasp.setuppinocchio(device=0)
    cq, cv = rc.traj_curves(d, int(d["ro_traj"][0]), bool(d["ro_vfile"][0]))
    trajs = (control.Curve(*cq), control.Curve(*cv))
    sim = control.Simulation(robot)
    sim.setqsim(d["ro_q0"][0], d["ro_v0"][0])
    tcur = float(d["ro_t0"][0])
    for k in range(4):
        control.controllaw(sim, robot, trajs, tcur, cube)
        tcur += 0.01
        q, v = sim.getpybulletstate()
        for name, x in (("q", q), ("v", v)):
            ref = d[f"ro_{name}_mp"]
            assert np.abs(x - ref[0, k]).max() <= d["tol_" + name][k] * np.abs(ref).max(), (name, k)
    r = control.rollout(robot, d["ro_q0"][:1], d["ro_v0"][:1], trajs, t0=d["ro_t0"][:1], ticks=4, record_every=1,
                        outputs=rc.HIST)
    assert np.array_equal(r["q_hist"][0], nextage_rollouts["q"][0, :4])
