"""Controller dynamics and torques on the GPU (control.py:284-406):
ikg_dynamics_batch and ikg_control_torque_batch against the fixtures of
tests/golden/dynamics_cases.npz (make_dynamics_golden.py).

Bounds: fp64 M / nle / g 1e-12 x max(1, max|fixture|); fp32 M / nle / g and
the controller outputs: the measured bounds stored in the fixture (tol32_*:
8 x the float32 oracle's error; tol_*: 20 x the float64 restatement's error
against the 50-digit evaluation, relative to max|output|).

The same kernels on every robot-family tree (nq = 13 ... 32, both lane groups,
both branches of tile_store): tests/test_gpu_dynamics_family.py."""
import os

import numpy as np
import pytest

import dynamics_oracle as do
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DYN = ("M", "nle", "g")
CTL = ("tau", "qdd", "xdd", "Lambda", "fc")


@pytest.fixture(scope="module")
def dc():
    return dict(np.load(os.path.join(GOLDEN, "dynamics_cases.npz")))


@pytest.fixture(scope="module")
def tilted_model():
    from ikgrasp.model import DualArmModel
    return DualArmModel.from_urdf(os.path.join(GOLDEN, "tilted_dualarm.urdf"), os.path.join(GOLDEN, "tilted_cube.urdf"))


@pytest.fixture(scope="module")
def full(solver, dc):
    """The B = 96 call every batch-shape and subset test compares against."""
    return solver.dynamics(dc["q"], dc["v"], outputs=DYN)


@pytest.fixture(scope="module")
def ctl(solver, dc):
    return solver.control_torques(dc["q"], dc["v"], dc["q_des"], dc["v_des"])


def _check_dynamics(r64, r32, dc, pre):
    for k in DYN:
        ref = dc[pre + k]
        e64 = np.abs(r64[k] - ref).max()
        e32 = np.abs(r32[k].astype(np.float64) - ref).max() / np.abs(ref).max()
        print(f"{pre}{k}: fp64 |d| {e64:.2e} (bound {1e-12 * max(1.0, np.abs(ref).max()):.1e}), "
              f"fp32 {e32:.2e} of max (bound {float(dc[pre + 'tol32_' + k]):.2e})")
        assert e64 <= 1e-12 * max(1.0, np.abs(ref).max()), k
        assert e32 <= float(dc[pre + "tol32_" + k]), k


def test_nextage_matches_fixtures(solver, dc, full):
    _check_dynamics(full, solver.dynamics(dc["q"], dc["v"], outputs=DYN, dtype="f32"), dc, "")


def test_tilted_model_matches_fixtures(dc, tilted_model):
    from ikgrasp.solver import IKSolver
    s = IKSolver(tilted_model, device=0, specialize=False)
    with pytest.raises(Exception, match="inertia"):  # an explicit model comes without inertias
        s.dynamics(dc["tilted_q"], dc["tilted_v"])
    s.set_inertia(do.seeded_inertias(tilted_model.nq, 1))
    r64 = s.dynamics(dc["tilted_q"], dc["tilted_v"], outputs=DYN)
    r32 = s.dynamics(dc["tilted_q"], dc["tilted_v"], outputs=DYN, dtype="f32")
    s.close()
    _check_dynamics(r64, r32, dc, "tilted_")


def test_output_handling(solver, dc, full):
    for k in DYN:
        assert np.array_equal(solver.dynamics(dc["q"], dc["v"], outputs=(k,))[k], full[k]), k
    r0 = solver.dynamics(dc["q"], None, outputs=("nle", "g"))
    assert np.array_equal(r0["nle"], r0["g"]) and np.array_equal(r0["g"], full["g"])
    assert np.array_equal(full["M"], full["M"].transpose(0, 2, 1))


@pytest.mark.parametrize("B", [1, 31, 33, 65, 96])
def test_batch_shapes(solver, dc, full, B):
    """Tile tails and more than one workgroup: the first B rows of the states
    tiled to 96 equal the same rows of the B = 96 call bit for bit."""
    r = solver.dynamics(dc["q"][:B], dc["v"][:B], outputs=DYN)
    c = solver.control_torques(dc["q"][:B], dc["v"][:B], dc["q_des"][:B], dc["v_des"][:B], outputs=("tau", "qdd"))
    ref = solver.control_torques(dc["q"], dc["v"], dc["q_des"], dc["v_des"], outputs=("tau", "qdd"))
    for k in DYN:
        assert r[k].shape[0] == B and np.array_equal(r[k], full[k][:B]), k
    for k in ("tau", "qdd"):
        assert np.array_equal(c[k], ref[k][:B]), k


def test_empty_batch_touches_nothing(solver):
    import ctypes as C
    from ikgrasp import _lib
    r = solver.dynamics(np.zeros((0, 15)), None, outputs=DYN)
    assert r["M"].shape == (0, 15, 15)
    guard = np.full(15, 7.0)
    out = _lib.DynamicsOut(None, guard.ctypes.data, None)
    assert solver.lib.ikg_dynamics_batch(solver._h, 0, 0, guard.ctypes.data, None, 0, C.byref(out), None,
                                         _lib.IKG_FLAG_HOST_POINTERS) == 0
    cout = _lib.ControlOut(guard.ctypes.data, None, None, None, None)
    prm = _lib.control_params()
    assert solver.lib.ikg_control_torque_batch(solver._h, 0, guard.ctypes.data, None, guard.ctypes.data, None, 0,
                                               C.byref(prm), C.byref(cout), None, _lib.IKG_FLAG_HOST_POINTERS) == 0
    assert np.all(guard == 7.0)


def test_passive_chain_below_an_arm_joint(tilted_model):
    """A tree that is not 'chest, head chain, two arms': the tilted robot's
    passive joint re-parented below an arm joint, seeded inertias, 16 states
    against the oracle."""
    from ikgrasp.solver import IKSolver
    m, _ = do.hanging_passive_model(tilted_model)
    assert m.parents[m.passive_q[0]] == m.arm_q[0][1]
    bi = do.seeded_inertias(m.nq, 5)
    rng = np.random.default_rng(11)
    q, v = rng.uniform(-1.5, 1.5, (16, m.nq)), rng.normal(0.0, 0.7, (16, m.nq))
    s = IKSolver(m, device=0, specialize=False)
    s.set_inertia(bi)
    r = s.dynamics(q, v, outputs=DYN)
    s.close()
    t = do.Tree(do.F64, m, bi)
    want = {"M": np.array([do.crba(t, x) for x in q]), "nle": np.array([do.nle(t, x, y) for x, y in zip(q, v)]),
            "g": np.array([do.gravity_torques(t, x) for x in q])}
    p = m.passive_q[0]
    assert np.abs(want["M"][:, p, m.arm_q[0][0]]).max() > 1e-3  # the passive body couples to the arm it hangs on
    for k in DYN:
        np.testing.assert_allclose(r[k], want[k], rtol=0, atol=1e-12 * max(1.0, np.abs(want[k]).max()), err_msg=k)


def test_control_torques_within_measured_bounds(solver, dc, ctl):
    for k in CTL:
        ref = dc[k + "_mp"]
        err = np.abs(ctl[k] - ref).max() / np.abs(ref).max()
        reg = ~dc["near_singular"]
        err_reg = np.abs(ctl[k][reg] - ref[reg]).max() / np.abs(ref[reg]).max()
        print(f"{k}: {err:.3e} of max|.| (bound {float(dc['tol_' + k]):.3e}); regular states {err_reg:.3e} "
              f"(bound {float(dc['tol_reg_' + k]):.3e})")
        assert err <= float(dc["tol_" + k]), k
    assert np.all(ctl["tau"][:, 1] == 0) and np.all(ctl["tau"][:, 2] == 0)
    assert np.all(ctl["qdd"][:, solver.model.passive_q] == 0)


def test_control_torques_across_scratch_chunks(solver, dc, ctl):
    """More states than one pass of the entry's scratch holds (65,536): every
    row equals the B = 96 call's row of the same state bit for bit."""
    B = 65536 + 97
    idx = np.arange(B) % 96
    r = solver.control_torques(dc["q"][idx], dc["v"][idx], dc["q_des"][idx], dc["v_des"][idx])
    for k in CTL:
        assert np.array_equal(r[k], ctl[k][idx]), k


def test_control_torques_honour_gains(solver, dc, ctl):
    g = dict(zip(("Kp", "Kv", "Kf", "Kt", "lambda_reg", "qp_reg"), dc["gains_alt"]))
    r = solver.control_torques(dc["q"][:8], dc["v"][:8], dc["q_des"][:8], dc["v_des"][:8], fc_bias=dc["fc_bias_alt"], **g)
    for k in CTL:
        ref = dc[k + "_alt_mp"]
        assert np.abs(r[k] - ref).max() <= float(dc["tol_" + k]) * np.abs(ref).max(), k
    assert np.abs(r["tau"] - ctl["tau"][:8]).max() > 1.0  # differs from the default answer
    z = solver.control_torques(dc["q"][:8], dc["v"][:8], dc["q_des"][:8], dc["v_des"][:8], zero_tau=(0, 14), outputs=("tau",))
    assert np.all(z["tau"][:, [0, 14]] == 0) and np.all(z["tau"][:, 2] != 0)


def test_host_and_device_calls_agree(solver, dc, full, ctl):
    import torch
    dev = lambda k: torch.tensor(dc[k], device="cuda", dtype=torch.float64)
    rd = solver.dynamics(dev("q"), dev("v"), outputs=DYN)
    rc = solver.control_torques(dev("q"), dev("v"), dev("q_des"), dev("v_des"))
    torch.cuda.synchronize()
    for k in DYN:
        assert np.array_equal(rd[k].cpu().numpy(), full[k]), k
    for k in CTL:
        assert np.array_equal(rc[k].cpu().numpy(), ctl[k]), k


def test_controllaw_dropin(dc, ctl):
    """The reference's signature and side effect with a stub simulator, at
    control points of the reference's trajectory.json (the first states of
    control_cases.npz)."""
    import ikgrasp
    from ikgrasp import control

    class Sim:
        def __init__(self, q, v):
            self.q, self.v, self.stepped = q, v, []

        def getpybulletstate(self):
            return list(self.q), list(self.v)

        def step(self, tau):
            self.stepped.append(tau)

    robot, _, _, cube = ikgrasp.setuppinocchio(device=0)
    for i in (0, 5, 17):
        sim = Sim(dc["q"][i], dc["v"][i])
        trajs = (lambda t, i=i: dc["q_des"][i], lambda t, i=i: dc["v_des"][i])
        assert control.controllaw(sim, robot, trajs, 0.25, cube) is None
        (tau,) = sim.stepped
        assert isinstance(tau, list) and len(tau) == 15 and all(isinstance(x, float) for x in tau)
        assert tau == ctl["tau"][i].tolist()
    b = control.control_torques_batch(robot, dc["q"][:4], dc["v"][:4], dc["q_des"][:4], dc["v_des"][:4])
    assert b["Lambda"].shape == (4, 2, 6, 6) and np.array_equal(b["tau"], ctl["tau"][:4])
    d = control.dynamics_terms_batch(robot, dc["q"][:4], dc["v"][:4])
    assert d["M"].shape == (4, 15, 15) and d["b"].shape == (4, 15)


def test_capture_and_replay_on_a_side_stream(solver, dc, ctl):
    import torch
    B = 33
    dev = lambda k: torch.tensor(dc[k][:B], device="cuda", dtype=torch.float64)
    q, v, qd, vd = dev("q"), dev("v"), dev("q_des"), dev("v_des")
    direct = solver.control_torques(q, v, qd, vd)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm up off the default stream, as torch recommends before capture
        solver.control_torques(q, v, qd, vd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # captures on a side stream, which is the current stream inside
        cap = solver.control_torques(q, v, qd, vd)
    for k in CTL:
        cap[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in CTL:
        assert np.array_equal(cap[k].cpu().numpy(), direct[k].cpu().numpy()), k
        assert np.array_equal(cap[k].cpu().numpy(), ctl[k][:B]), k
    del graph
