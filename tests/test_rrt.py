"""RRT-Connect planner on the CPU (tests/golden/rrt_cases.npz, made by
tests/golden/make_rrt_golden.py with tests/rrt_oracle.py):

  * the fixtures replay from their seeds (the reference's draw order);
  * get_path on hand-built trees, duplicate vertices included;
  * the planner step (ikgrasp.path.rrt_iteration / rrt_connect), driven by
    callables that replay the recorded samples and segments, rebuilds the
    recorded trees and path exactly;
  * the emulator's SE3.Interpolate (the kernel's device function on the host)
    against the 50-digit values;
  * the emulator's nearest rule (per-row distance, argmin combine), ties included.

The projection's own bookkeeping (prepare / commit per chain, the step loop) on
the emulator is tests/test_projection.py, on tests/golden/projection_cases.npz
(tests/golden/make_projection_golden.py, tests/projection_cases.py).
"""
import numpy as np
import pytest

import emu as host_emu
import rrt_cases as rc

STEP = 0.025


@pytest.fixture(scope="module")
def cases():
    return rc.rrt_cases()


@pytest.fixture(scope="module")
def emu():
    return host_emu.load()


def emu_nearest(lib, nodes, counts, queries):
    nodes, queries = np.ascontiguousarray(nodes, dtype=np.float64), np.ascontiguousarray(queries, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    P, cap, nq = nodes.shape
    idx, dist = np.empty(P, dtype=np.int32), np.empty(P)
    assert lib.ikg_emu_nearest(nodes.ctypes.data, cap, counts.ctypes.data, queries.ctypes.data, nq, P,
                               idx.ctypes.data, dist.ctypes.data) == 0
    return idx, dist


def _replay_stream(c, prefix, seed, t0, t1):
    """Walk the case's RandomState as the reference would; returns the next draw."""
    rs = np.random.RandomState(seed)
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    for i in range(len(c[f"{prefix}_bias"])):
        assert bool(rs.rand() < 0.1) == bool(c[f"{prefix}_bias"][i])
        if c[f"{prefix}_bias"][i]:
            continue
        for _ in range(1000):
            t = np.array([rs.uniform(lo[0], hi[0]), rs.uniform(lo[1], hi[1]), rs.uniform(1.05, 1.4)])
            if np.array_equal(t, c[f"{prefix}_t_rand"][i]):
                break
        else:
            raise AssertionError("the recorded sample is not in the stream")
    return rs.random_sample()


@pytest.mark.parametrize("seed", rc.M_SEEDS)
def test_fixture_replays_from_its_seed(cases, seed):
    c = cases
    assert _replay_stream(c, f"M{seed}", seed, c["M_t0"], c["M_t1"]) == c[f"M{seed}_next"]
    # a goal-biased iteration samples the goal itself
    for i in np.nonzero(c[f"M{seed}_bias"])[0]:
        assert np.array_equal(c[f"M{seed}_q_rand"][i], c["M_qgoal"])
        assert np.array_equal(c[f"M{seed}_t_rand"][i], c["M_t1"])
    assert c[f"M{seed}_connect"][-1] < 0.5 and (c[f"M{seed}_connect"][:-1] >= 0.5).all()
    assert np.array_equal(c[f"M{seed}_path"][0], c["M_qinit"]) and np.array_equal(c[f"M{seed}_path"][-1], c["M_qgoal"])


def test_fixture_r_replays_and_fails(cases):
    c = cases
    assert _replay_stream(c, "R", 0, c["R_t0"], c["R_t1"]) == c["R_next"]
    assert len(c["R_bias"]) == 3 and (c["R_connect"] >= 0.5).all() and c["R_path"].shape[0] == 0
    # after iteration 0 the start tree has 5 vertices (root + the first segment)
    assert 1 + c["R_seg_start_n"][0] == 5
    assert np.array_equal(c["proj_status"], [0, 2])


def test_get_path_on_hand_built_trees():
    from ikgrasp.path import get_path
    assert get_path([(None, "a")]) == ["a"]
    # a chain, a branch that is not on the way, and the last vertex under the chain
    G = [(None, "r"), (0, "a"), (1, "b"), (0, "x"), (2, "c")]
    assert get_path(G) == ["r", "a", "b", "c"]
    # duplicates as the planner makes them: a segment repeats its start vertex
    G = [(None, "r"), (0, "r"), (1, "a"), (2, "b"), (3, "b"), (4, "c")]
    assert get_path(G) == ["r", "r", "a", "b", "b", "c"]
    # the same tree with the duplicate's children under the first copy: fewer repeats, the same vertices
    G2 = [(None, "r"), (0, "r"), (0, "a"), (2, "b"), (3, "b"), (3, "c")]
    assert get_path(G2) == ["r", "a", "b", "c"]
    assert [x for k, x in enumerate(get_path(G)) if k == 0 or get_path(G)[k - 1] != x] == get_path(G2)


def _replay_planner(c, prefix, qinit, qgoal, t0, t1, nearest, **kw):
    """rrt_connect on host trees with the recorded samples and segments."""
    from ikgrasp.path import Trees, rrt_connect
    trees = Trees([qinit], [qgoal], rc.rows12(t0), rc.rows12(t1), cap=4)  # grows on the way
    state = {"it": 0, "seg": 0, "off": {"start": 0, "goal": 0}}

    def sample(planners):
        i = state["it"]
        return c[f"{prefix}_q_rand"][i][None], rc.rows12(c[f"{prefix}_t_rand"][i])

    def project(q_near, cube_near, cube_to):
        side = ("start", "goal")[state["seg"] % 2]
        i = state["seg"] // 2
        n, off = int(c[f"{prefix}_seg_{side}_n"][i]), state["off"][side]
        seg_q = c[f"{prefix}_seg_{side}_q"][off:off + n]
        seg_t = c[f"{prefix}_seg_{side}_t"][off:off + n]
        # the recorded segment starts at the vertex the step chose, and heads where it says
        assert np.array_equal(seg_q[0], q_near[0]) and np.array_equal(seg_t[0], cube_near[0, 9:])
        want = c[f"{prefix}_t_rand"][i] if side == "start" else t1
        assert np.array_equal(cube_to[0, 9:], want)
        state["off"][side] += n
        state["seg"] += 1
        if side == "goal":
            state["it"] += 1
        return seg_q[None], rc.rows12(seg_t)[None], np.array([n])

    def connect(q_a, q_b):
        return np.linalg.norm(q_b - q_a, axis=1)

    paths = rrt_connect(trees, sample, nearest, project, connect, **kw)
    return paths[0], trees.export(0), state["it"]


def _check_trees(c, prefix, tr):
    for side in ("start", "goal"):
        assert np.array_equal(tr[f"{side}_parent"], c[f"{prefix}_{side}_parent"])
        assert np.array_equal(tr[f"{side}_q"], c[f"{prefix}_{side}_q"])
        assert np.array_equal(tr[f"{side}_cube"][:, 9:], c[f"{prefix}_{side}_t"])


@pytest.mark.parametrize("seed", rc.M_SEEDS)
def test_planner_step_rebuilds_recorded_trees_and_path(cases, emu, seed):
    c = cases

    def nearest(trees, side, planners, queries):  # the kernel's rule, on the host
        return emu_nearest(emu, trees.q[side], trees.count[side], queries)[0]

    path, tr, its = _replay_planner(c, f"M{seed}", c["M_qinit"], c["M_qgoal"], c["M_t0"], c["M_t1"], nearest)
    assert its == len(c[f"M{seed}_bias"])
    _check_trees(c, f"M{seed}", tr)
    assert np.array_equal(np.array(path), c[f"M{seed}_path"])


def test_planner_step_failing_query_keeps_last_trees(cases):
    c = cases

    def nearest(trees, side, planners, queries):
        return rc.nearest_reference(trees.q[side], trees.count[side], queries)[0]

    path, tr, its = _replay_planner(c, "R", c["R_qinit"], c["R_qgoal"], c["R_t0"], c["R_t1"], nearest,
                                    max_iterations=3, max_retries=1)
    assert path == [] and its == 3
    _check_trees(c, "R", tr)


def test_recorded_nearest_indices_follow_the_lowest_index_rule(cases):
    """Each recorded query, asked again of the recorded tree's prefix."""
    c = cases
    for seed in rc.M_SEEDS:
        p = f"M{seed}"
        n = 1
        for i in range(len(c[f"{p}_bias"])):
            idx, _ = rc.nearest_reference(c[f"{p}_start_q"][None, :n], [n], c[f"{p}_q_rand"][i][None])
            assert idx[0] == c[f"{p}_near"][i, 0]
            n += int(c[f"{p}_seg_start_n"][i])


def test_emulator_interpolate_matches_50_digits(cases, emu):
    c = cases
    A, B, al = c["interp_A"], c["interp_B"], c["interp_alpha"]
    out = host_emu.se3_interpolate(A, B, al)
    err = np.abs(out - c["interp_exact"]).max(axis=1)
    bound = np.maximum(16 * c["interp_err"], 1e-15)
    print("interpolate: emulator error", err.tolist(), "bound", bound.tolist())
    assert (err <= bound).all()
    # identity rotations: the lerp
    for k in np.nonzero(c["interp_angle"] == 0.0)[0]:
        lerp = A[k, 9:] + al[k] * (B[k, 9:] - A[k, 9:])
        assert np.abs(out[k, 9:] - lerp).max() <= 1e-15 and np.array_equal(out[k, :9], np.eye(3).reshape(9))
    # every fixture angle is there, on both sides of the Taylor threshold eps^(1/4)
    assert set(c["interp_angle"]) == {0.0, 1e-5, 2e-4, 1.0, 3.0} and 1e-5 < np.finfo(float).eps ** 0.25 < 2e-4


@pytest.mark.parametrize("case", rc.nearest_cases(), ids=lambda x: x[0])
def test_emulator_nearest_rule(emu, case):
    _, nodes, counts, queries = case
    idx, dist = emu_nearest(emu, nodes, counts, queries)
    ref_idx, ref_dist = rc.nearest_reference(nodes, counts, queries)
    assert np.array_equal(idx, ref_idx)
    # nq products, nq sums and a square root, each within half an ulp
    assert (np.abs(dist - ref_dist) <= (nodes.shape[2] + 2) * np.finfo(float).eps * ref_dist).all()
    assert (idx < counts).all()  # never a row past the count (they hold the query itself)


def test_emulator_nearest_ties_go_to_the_lowest_index(emu):
    name, nodes, counts, queries = [x for x in rc.nearest_cases() if x[0] == "duplicates"][0]
    idx, _ = emu_nearest(emu, nodes, counts, queries)
    assert list(idx) == [6, 5]
    name, nodes, counts, queries = [x for x in rc.nearest_cases() if x[0] == "all_equal"][0]
    assert list(emu_nearest(emu, nodes, counts, queries)[0]) == [0]
    name, nodes, counts, queries = [x for x in rc.nearest_cases() if x[0] == "empty"][0]
    assert emu_nearest(emu, nodes, counts, queries)[0][0] == -1
