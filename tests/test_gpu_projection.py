"""Device-side path projection (ikg_project_paths) on the GPU against
tests/golden/projection_cases.npz (tests/golden/make_projection_golden.py;
shared code and the bars in tests/projection_cases.py; the CPU leg on the host
emulator is tests/test_projection.py):

  a. each chain alone, host pointers, max_nodes = steps + 2: the oracle's
     n_nodes and status, q within 1e-9 of its rows, cube rows within max(16 x
     the float64 restatement's recorded error, 1e-15) of the 50-digit rows
     (identity rotations 1e-15), rows at and past n_nodes zero, no live status;
  b. each step-size group in one launch, in fixture order and in a fixed
     permutation: per chain the same n_nodes / status as alone, q within 1e-12,
     cube rows bitwise;
  c. C = 1, 31, 33, 65, 257 chains, the group tiled so that wave neighbours
     differ in outcome: every copy equals its chain's answer of (a);
  d. the device-pointer route: ROCm tensors on a side stream, max_nodes =
     longest + 8 (max_nodes - 1 steps enqueued, no memset, finished chains idle):
     the host-pointer call's n_nodes / status, its rows below n_nodes bitwise,
     no live status, the inputs unchanged;
  e. the max_nodes edges (projection_cases.check_max_nodes_edges);
  f. the step boundary: |dt| / step_size an integer k gives k + 1 steps; just
     below it, k steps and a spare step of the host that changes nothing;
  g. ikgrasp.path.project_paths on both routes on the new chains, and where
     they leave the cube for one chain of each status;
  h. the refusals, which leave pre-filled outputs untouched.
"""
import ctypes as C

import numpy as np
import pytest

import projection_cases as pj

pytestmark = pytest.mark.gpu

NAMES = pj.names()


@pytest.fixture(scope="module")
def robot_cube():
    import ikgrasp
    robot, _, _, cube = ikgrasp.setuppinocchio()
    return robot, cube


@pytest.fixture(scope="module")
def run(robot_cube):
    s = robot_cube[0].solver

    def call(q0, A, B, step_size, max_nodes):
        return s.project_paths(q0, A, B, step_size=step_size, max_nodes=max_nodes, **pj.SOLVE)

    return call


@pytest.fixture(scope="module")
def alone(run):
    """(a)'s answers, computed once: every chain alone at max_nodes = steps + 2."""
    return [pj.run_alone(run, i) for i in range(len(NAMES))]


@pytest.mark.parametrize("name", NAMES)
def test_each_chain_alone(alone, name):
    i = pj.index(name)
    dq, ce = pj.compare(i, alone[i])
    print(f"{name}: |dq| vs oracle {dq:.2e}, cube-row error / bound {ce:.2f}")


@pytest.mark.parametrize("order", ["fixture", "permuted"])
@pytest.mark.parametrize("which", ["main", "boundary"])
def test_one_launch_mixed_outcomes(run, alone, which, order):
    idx = pj.group(which) if order == "fixture" else pj.permuted(which)
    res = pj.run_batch(run, which, idx)
    for j, i in enumerate(idx):
        got = pj.chain_of(res, j)
        pj.compare(i, got)
        pj.same(got, alone[i])


@pytest.mark.parametrize("n_chains", [1, 31, 33, 65, 257])
def test_batch_shapes(run, alone, n_chains):
    idx = pj.tiled("main", n_chains)
    res = pj.run_batch(run, "main", idx)
    assert (res["status"] != pj.LIVE).all()
    for j, i in enumerate(idx):
        got = pj.chain_of(res, j)
        pj.same(got, alone[i])
        n = int(got["n_nodes"])
        assert not got["robot_path"][n:].any() and not got["cube_path"][n:].any()


def test_device_pointer_route(robot_cube, run):
    import torch
    s = robot_cube[0].solver
    idx = pj.permuted("main")
    q0, A, B = pj.inputs(idx)
    M = pj.longest(idx) + 8
    host = run(q0, A, B, pj.step_size("main"), M)
    dev = torch.device("cuda", s.device)
    tq, ta, tb = (torch.as_tensor(x, device=dev) for x in (q0, A, B))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        res = s.project_paths(tq, ta, tb, step_size=pj.step_size("main"), max_nodes=M, **pj.SOLVE)
    side.synchronize()
    n_nodes, status = res["n_nodes"].cpu().numpy(), res["status"].cpu().numpy()
    assert np.array_equal(n_nodes, host["n_nodes"]) and np.array_equal(status, host["status"])
    assert (status != pj.LIVE).all()
    rp, cp = res["robot_path"].cpu().numpy(), res["cube_path"].cpu().numpy()
    for j in range(len(idx)):  # the rows past n_nodes are unspecified on this route: not read
        n = int(n_nodes[j])
        assert np.array_equal(rp[j, :n], host["robot_path"][j, :n]) and np.array_equal(cp[j, :n], host["cube_path"][j, :n])
    for t, x in ((tq, q0), (ta, A), (tb, B)):
        assert np.array_equal(t.cpu().numpy(), x)


def test_max_nodes_edges(run):
    pj.check_max_nodes_edges(run)


def test_step_boundary(run, alone):
    c = pj.cases()
    for name in ("b1", "b4"):
        i = pj.index(name)
        k = int(c["k"][i])
        assert c["steps"][i] == k + 1
        assert (int(alone[i]["n_nodes"]), int(alone[i]["status"])) == (k + 2, pj.REACHED)
    # b4s, just below the integer: 4 steps on the device, 5 enqueued by the host; with
    # room for 4 steps only (max_nodes = 5) the same rows
    i = pj.index("b4s")
    assert (int(alone[i]["n_nodes"]), int(alone[i]["status"])) == (5, pj.REACHED)
    q0, A, B = pj.inputs([i])
    tight = pj.chain_of(run(q0, A, B, pj.step_size("boundary"), 5), 0)
    pj.same(tight, alone[i], tol=0.0)


def _se3_lists(idx):
    from ikgrasp.se3 import SE3
    q0, A, B = pj.inputs(idx)
    return ([q for q in q0], [SE3(a[:9].reshape(3, 3), a[9:]) for a in A], [SE3(b[:9].reshape(3, 3), b[9:]) for b in B])


def _as_answer(rp, cp):
    cube = np.array([np.concatenate([np.asarray(p.rotation).reshape(9), np.asarray(p.translation)]) for p in cp])
    return {"robot_path": np.array(rp), "cube_path": cube, "n_nodes": len(rp), "status": None}


@pytest.mark.parametrize("on_device", [False, True], ids=["host_route", "device_route"])
@pytest.mark.parametrize("which", ["main", "boundary"])
def test_project_paths_routes_meet_the_oracle(robot_cube, which, on_device):
    from ikgrasp.path import project_paths
    idx = pj.group(which)
    paths = project_paths(robot_cube[0], *_se3_lists(idx), step_size=pj.step_size(which), on_device=on_device)
    worst = 0.0
    for i, (rp, cp) in zip(idx, paths):
        assert len(rp) == len(cp)
        dq, _ = pj.compare(i, _as_answer(rp, cp), tail_zero=False)
        worst = max(worst, dq)
    print(f"{which}, on_device={on_device}: largest |dq| vs oracle {worst:.2e}")


@pytest.mark.parametrize("name", ["rz", "obst_rz", "up"])
def test_project_paths_leaves_the_cube_at_the_last_attempt(robot_cube, name):
    """One chain of status 0, 1 and 2 with a `cube`: after the call cube.placement
    is Interpolate(min(len, steps) / steps) on both routes (the reference sets
    the cube before the placement check, so a colliding attempt counts)."""
    from ikgrasp.path import project_paths
    from ikgrasp.se3 import interpolate
    robot, cube = robot_cube
    c, i = pj.cases(), pj.index(name)
    qs, a, b = _se3_lists([i])
    steps = int(c["steps"][i])
    left = []
    for on_device in (False, True):
        (rp, cp), = project_paths(robot, qs, a, b, step_size=float(c["step_size"][i]), cube=cube, on_device=on_device)
        pj.compare(i, _as_answer(rp, cp), tail_zero=False)
        want = interpolate(a[0], b[0], min(len(rp), steps) / steps)
        got = cube.placement
        assert np.array_equal(np.asarray(got.rotation), np.asarray(want.rotation)), (name, on_device)
        assert np.array_equal(np.asarray(got.translation), np.asarray(want.translation)), (name, on_device)
        left.append(got)
    assert np.array_equal(np.asarray(left[0].translation), np.asarray(left[1].translation))
    assert np.array_equal(np.asarray(left[0].rotation), np.asarray(left[1].rotation))


def test_refusals_leave_the_outputs(robot_cube):
    from ikgrasp import _lib
    s = robot_cube[0].solver
    q0, A, B = pj.inputs(pj.group("main")[:2])
    env = np.ascontiguousarray(s.scene.env_geoms(), dtype=np.int32)
    target = next(k for k, g in enumerate(s.scene.geoms) if g.target)
    prm = s.params(**pj.SOLVE)
    far = B.copy()
    far[1, 9] += 3e7  # |dt| / step_size >= 1e9
    for kw in (dict(step_size=0.0), dict(step_size=-0.025), dict(max_nodes=0),
               dict(geoms=np.array([env[0], target], dtype=np.int32)), dict(B=far)):
        a = dict(q0=q0, A=A, B=B, step_size=0.025, max_nodes=4, geoms=env)
        a.update(kw)
        rp, cp = np.full((2, 4, 15), 7.5), np.full((2, 4, 12), 7.5)
        nn, st = np.full(2, 77, dtype=np.int32), np.full(2, 77, dtype=np.int32)
        with pytest.raises(_lib.IkgError):
            _lib.check(s.lib.ikg_project_paths(s._h, s.device, a["q0"].ctypes.data, a["A"].ctypes.data, a["B"].ctypes.data, 2,
                                               float(a["step_size"]), int(a["max_nodes"]), a["geoms"].ctypes.data,
                                               a["geoms"].size, C.byref(prm), rp.ctypes.data, cp.ctypes.data,
                                               nn.ctypes.data, st.ctypes.data, None, _lib.IKG_FLAG_HOST_POINTERS))
        assert (rp == 7.5).all() and (cp == 7.5).all() and (nn == 77).all() and (st == 77).all(), kw
