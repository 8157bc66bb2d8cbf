"""RRT-Connect planner on the GPU against tests/golden/rrt_cases.npz
(tests/golden/make_rrt_golden.py, tests/rrt_oracle.py):

  1. ikg_se3_interpolate_batch against the 50-digit values: within 16 x the
     float64 restatement's own recorded error (floor 1e-15; the factor covers
     fused and reordered sums), identity rotations within 1e-15 of the lerp;
  2. ikg_nearest_batch against numpy on counts around the wave size, three row
     lengths, unequal trees under a larger cap, rows past the count that equal
     the query, bitwise duplicates (lowest index);
  3. project_paths(on_device=True) on the chains path, pathb, path of
     planner_cases.npz: the host route's lengths, q within 1e-12 of it and 1e-9
     of the fixture, translations within 1e-15, the recorded status; max_nodes=4
     cuts `path` at 4 nodes with status 3;
  4. computepath on query M (RandomState seeds 3, 4, 6): the fixture's path
     once consecutive equal rows are removed (q within 1e-9), equal tree
     parents, the same next draw; on R no path and equal trees; robot=None: [];
  5. computepaths: three planners on M connect, each as when run alone, every
     node collision-free, ends at qinit / qgoal;
  6. a planned path goes through ikgrasp.control.maketraj.

The projection on every chain outcome (statuses 0 / 1 / 2 / 3, stops after
accepted nodes, rotated goals, batch shapes, the device-pointer route, the
max_nodes edges) is tests/test_gpu_projection.py on
tests/golden/projection_cases.npz; its CPU leg is tests/test_projection.py.
"""
import os

import numpy as np
import pytest

import rrt_cases as rc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return rc.rrt_cases()


@pytest.fixture(scope="module")
def pc():
    return dict(np.load(os.path.join(GOLDEN, "planner_cases.npz")))


@pytest.fixture(scope="module")
def robot_cube():
    import ikgrasp
    robot, _, _, cube = ikgrasp.setuppinocchio()
    return robot, cube


def _m_query(c):
    from ikgrasp.se3 import SE3
    return c["M_qinit"], c["M_qgoal"], SE3(np.eye(3), c["M_t0"]), SE3(np.eye(3), c["M_t1"])


def test_se3_interpolate_matches_50_digits(robot_cube, cases):
    import torch
    s, c = robot_cube[0].solver, cases
    out = s.se3_interpolate(c["interp_A"], c["interp_B"], c["interp_alpha"])
    err = np.abs(out - c["interp_exact"]).max(axis=1)
    bound = np.maximum(16 * c["interp_err"], 1e-15)
    print("interpolate: device error", err.tolist(), "bound", bound.tolist())
    assert (err <= bound).all()
    for k in np.nonzero(c["interp_angle"] == 0.0)[0]:
        lerp = c["interp_A"][k, 9:] + c["interp_alpha"][k] * (c["interp_B"][k, 9:] - c["interp_A"][k, 9:])
        assert np.abs(out[k, 9:] - lerp).max() <= 1e-15 and np.abs(out[k, :9] - np.eye(3).reshape(9)).max() <= 1e-15
    # device tensors: the same numbers
    dev = torch.device("cuda", s.device)
    t = lambda x: torch.as_tensor(x, device=dev)
    out_t = s.se3_interpolate(t(c["interp_A"]), t(c["interp_B"]), t(c["interp_alpha"]))
    assert np.array_equal(out_t.cpu().numpy(), out)


@pytest.mark.parametrize("case", rc.nearest_cases(), ids=lambda x: x[0])
def test_nearest_matches_numpy(robot_cube, case):
    s = robot_cube[0].solver
    _, nodes, counts, queries = case
    idx, dist = s.nearest(nodes, counts, queries)
    ref_idx, ref_dist = rc.nearest_reference(nodes, counts, queries)
    assert np.array_equal(idx, ref_idx)
    assert (idx < counts).all()  # the rows past the count hold the query itself
    # nq products, nq sums (fused on the device) and a square root, each within half an ulp
    assert (np.abs(dist - ref_dist) <= (nodes.shape[2] + 2) * np.finfo(float).eps * ref_dist).all()


def test_nearest_ties_and_device_tensors(robot_cube):
    import torch
    s = robot_cube[0].solver
    by_name = {x[0]: x[1:] for x in rc.nearest_cases()}
    assert list(s.nearest(*by_name["duplicates"])[0]) == [6, 5]
    assert list(s.nearest(*by_name["all_equal"])[0]) == [0]
    assert list(s.nearest(*by_name["empty"])[0])[0] == -1
    dev = torch.device("cuda", s.device)
    nodes, counts, queries = by_name["P3_unequal"]
    idx, dist = s.nearest(torch.as_tensor(nodes, device=dev), torch.as_tensor(counts, device=dev),
                          torch.as_tensor(queries, device=dev))
    ref = s.nearest(nodes, counts, queries)
    assert np.array_equal(idx.cpu().numpy(), ref[0]) and np.array_equal(dist.cpu().numpy(), ref[1])


def test_project_paths_on_device(robot_cube, pc, cases):
    from ikgrasp.path import project_paths
    from ikgrasp.se3 import SE3
    robot, _ = robot_cube
    keys = ["path", "pathb", "path"]
    q0 = [pc[f"{k}_start_q"] for k in keys]
    a = [SE3(np.eye(3), pc[f"{k}_start_t"]) for k in keys]
    b = [SE3(np.eye(3), pc[f"{k}_goal_t"]) for k in keys]
    host = project_paths(robot, q0, a, b)
    dev = project_paths(robot, q0, a, b, on_device=True)
    for k, (rp, cp), (hp, hc) in zip(keys, dev, host):
        assert len(rp) == len(hp) == len(cp) == len(pc[f"{k}_q"])
        dq_host, dq_fix = np.abs(np.array(rp) - np.array(hp)).max(), np.abs(np.array(rp) - pc[f"{k}_q"]).max()
        dt = np.abs(np.array([p.translation for p in cp]) - pc[f"{k}_t"]).max()
        print(f"{k}: |dq| vs host route {dq_host:.2e}, vs fixture {dq_fix:.2e}, |dt| {dt:.2e}")
        assert dq_host <= 1e-12 and dq_fix <= 1e-9 and dt <= 1e-15
    s = robot.solver
    from ikgrasp.se3 import pack_targets
    res = s.project_paths(np.array(q0), pack_targets(a), pack_targets(b), max_nodes=len(pc["path_q"]) + 2,
                          eps=1e-3, dt=1e-2, max_iters=1000)
    want = [int(cases["proj_status"][0]), int(cases["proj_status"][1]), int(cases["proj_status"][0])]
    assert list(res["status"]) == want
    assert list(res["n_nodes"]) == [len(pc[f"{k}_q"]) for k in keys]
    cut = s.project_paths(np.array(q0), pack_targets(a), pack_targets(b), max_nodes=4)
    assert list(cut["n_nodes"]) == [4, 1, 4] and list(cut["status"]) == [3, want[1], 3]
    assert np.array_equal(cut["robot_path"][0], res["robot_path"][0, :4])


@pytest.mark.parametrize("seed", rc.M_SEEDS)
def test_computepath_matches_the_oracle(robot_cube, cases, seed):
    import ikgrasp
    robot, cube = robot_cube
    c = cases
    np.random.seed(seed)
    path, tr = ikgrasp.computepath(*_m_query(c), robot=robot, cube=cube, return_trees=True)
    assert np.random.random_sample() == c[f"M{seed}_next"]
    got, want = rc.dedup(path), rc.dedup(c[f"M{seed}_path"])
    assert len(got) == len(want)
    dq = np.abs(np.array(got) - np.array(want)).max()
    print(f"seed {seed}: {len(path)} rows ({len(got)} distinct), |dq| vs fixture {dq:.2e}")
    assert dq <= 1e-9
    for side in ("start", "goal"):
        assert np.array_equal(tr[f"{side}_parent"], c[f"M{seed}_{side}_parent"])
        assert np.abs(tr[f"{side}_q"] - c[f"M{seed}_{side}_q"]).max() <= 1e-9


def test_computepath_without_a_path_and_without_a_robot(robot_cube, cases):
    import ikgrasp
    from ikgrasp.se3 import SE3
    robot, cube = robot_cube
    c = cases
    np.random.seed(0)
    path, tr = ikgrasp.computepath(c["R_qinit"], c["R_qgoal"], SE3(np.eye(3), c["R_t0"]), SE3(np.eye(3), c["R_t1"]),
                                   robot=robot, cube=cube, max_iterations=3, max_retries=1, return_trees=True)
    assert path == []
    assert np.random.random_sample() == c["R_next"]
    for side in ("start", "goal"):
        assert np.array_equal(tr[f"{side}_parent"], c[f"R_{side}_parent"])
        assert np.abs(tr[f"{side}_q"] - c[f"R_{side}_q"]).max() <= 1e-9
        assert np.abs(tr[f"{side}_cube"][:, 9:] - c[f"R_{side}_t"]).max() <= 1e-15
    assert ikgrasp.computepath(*_m_query(c), robot=None, cube=cube) == []
    assert ikgrasp.computepath(*_m_query(c), robot=robot, cube=None) == []


@pytest.fixture(scope="module")
def lockstep(robot_cube, cases):
    import ikgrasp
    robot, _ = robot_cube
    qi, qg, a, b = _m_query(cases)
    seeds = [11, 12, 13]
    paths, trees = ikgrasp.computepaths(robot, [qi] * 3, [qg] * 3, [a] * 3, [b] * 3, seeds, return_trees=True)
    return seeds, paths, trees


def test_computepaths_equals_each_planner_alone(robot_cube, cases, lockstep):
    import ikgrasp
    robot, _ = robot_cube
    qi, qg, a, b = _m_query(cases)
    seeds, paths, trees = lockstep
    assert all(len(p) > 0 for p in paths)
    for k, seed in enumerate(seeds):
        (one,), (tr,) = ikgrasp.computepaths(robot, [qi], [qg], [a], [b], [seed], return_trees=True)
        assert len(one) == len(paths[k])
        assert np.abs(np.array(one) - np.array(paths[k])).max() <= 1e-12
        for side in ("start", "goal"):
            assert np.array_equal(tr[f"{side}_parent"], trees[k][f"{side}_parent"])
            assert np.abs(tr[f"{side}_q"] - trees[k][f"{side}_q"]).max() <= 1e-12


def test_computepaths_nodes_are_collision_free(robot_cube, cases, lockstep):
    robot, _ = robot_cube
    c = cases
    _, paths, trees = lockstep
    for path, tr in zip(paths, trees):
        assert np.array_equal(path[0], c["M_qinit"]) and np.array_equal(path[-1], c["M_qgoal"])
        for side in ("start", "goal"):  # every tree vertex, the path's among them, with the cube where it was grasped
            assert not robot.solver.collision(tr[f"{side}_q"], tr[f"{side}_cube"]).any()
        rows = {q.tobytes() for side in ("start", "goal") for q in tr[f"{side}_q"]}
        assert all(np.asarray(q).tobytes() in rows for q in path)


def test_path_goes_through_maketraj(lockstep):
    from ikgrasp.control import maketraj
    _, paths, _ = lockstep
    path = np.array(paths[0])
    (q_of_t, vq_of_t, vvq_of_t), _ = maketraj(path[0], path[-1], path, 1.0)
    # the curve's ends are pinned to the path's (control.py:63-197)
    assert np.abs(np.asarray(q_of_t(0.0)) - path[0]).max() <= 1e-12
    assert np.abs(np.asarray(q_of_t(1.0)) - path[-1]).max() <= 1e-12
    assert np.isfinite(np.asarray(q_of_t(0.5))).all() and np.asarray(vq_of_t(0.5)).shape == path[0].shape
