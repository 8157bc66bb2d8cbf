"""Shared code of tests/test_projection.py (host emulator) and
tests/test_gpu_projection.py (ikg_project_paths on the GPU): the fixture
tests/golden/projection_cases.npz (tests/golden/make_projection_golden.py),
batch builders and the comparison with the oracle (test infrastructure).

A leg gives `run(q0 [C,nq], A [C,12], B [C,12], step_size, max_nodes)` -> dict
of robot_path [C,M,nq], cube_path [C,M,12], n_nodes [C], status [C] (numpy):
one host-pointer call of the projection.

A call has one step_size, so the chains form two groups: "main" (0.025) and
"boundary" (2^-5).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOLVE = dict(eps=1e-3, dt=1e-2, max_iters=1000, check_collision=True)  # the planner's solve (ikgrasp/path.py)
Q_TOL = 1e-9  # the project's fp64 IK bar against the oracle (tests/test_gpu_planner.py)
SAME_TOL = 1e-12  # the same kernels from the same warm starts (test_project_paths_batch_equals_dropin)
LIVE, REACHED, COLLISION, IK_FAILED, CUT = -1, 0, 1, 2, 3

_cache = {}


def cases():
    if "c" not in _cache:
        _cache["c"] = dict(np.load(os.path.join(GOLDEN, "projection_cases.npz")))
    return _cache["c"]


def names():
    return [str(n) for n in cases()["names"]]


def index(name):
    return names().index(name)


def group(which):
    """Chain indices of "main" (step_size 0.025) or "boundary" (2^-5), in fixture order."""
    k = cases()["k"]
    return [i for i in range(len(k)) if (k[i] >= 0) == (which == "boundary")]


def step_size(which):
    c = cases()
    s = {float(c["step_size"][i]) for i in group(which)}
    assert len(s) == 1
    return s.pop()


def longest(idx):
    return int(max(cases()["steps"][i] for i in idx))


def rows(i):
    """(q [n,nq], cube rows in 50 digits [n,12], the float64 restatement's error [n]) of chain i"""
    c = cases()
    a, b = int(c["row_off"][i]), int(c["row_off"][i + 1])
    return c["q"][a:b], c["cube_exact"][a:b], c["cube_err"][a:b]


def inputs(idx):
    c = cases()
    idx = list(idx)
    return (np.ascontiguousarray(c["q0"][idx]), np.ascontiguousarray(c["A"][idx]), np.ascontiguousarray(c["B"][idx]))


def permuted(which):
    """A fixed order of the group in which neighbours differ in outcome: the
    chains sorted by (status, n_nodes) dealt round-robin over the statuses."""
    c = cases()
    by = {s: [i for i in group(which) if c["status"][i] == s] for s in (0, 1, 2)}
    out = []
    while any(by.values()):
        for s in (2, 0, 1):
            if by[s]:
                out.append(by[s].pop())
    return out


def tiled(which, C):
    """C chain indices: the permuted group repeated, each round rotated by one
    more place so that a copy's lane and wave neighbours change from round to round."""
    base = permuted(which)
    out, r = [], 0
    while len(out) < C:
        out += base[r % len(base):] + base[:r % len(base)]
        r += 1
    return out[:C]


def chain_of(res, j):
    return {k: res[k][j] for k in ("robot_path", "cube_path", "n_nodes", "status")}


def compare(i, got, q_tol=Q_TOL, tail_zero=True):
    """One chain's answer (chain_of) against the fixture: n_nodes and status
    equal (never live); q rows within q_tol of the oracle's; cube rows within max(16 x the
    recorded float64 error, 1e-15) of the 50-digit rows (the rule of
    test_se3_interpolate_matches_50_digits), identity-rotation chains within
    1e-15; rows at and past n_nodes zero.  -> (largest |dq|, largest cube-row
    error over its bound)."""
    c = cases()
    name = names()[i]
    q, cube, err = rows(i)
    n = int(got["n_nodes"])
    if got.get("status") is not None:  # (the list-returning routes of ikgrasp.path report no status)
        assert int(got["status"]) != LIVE, name
        assert int(got["status"]) == int(c["status"][i]), (name, int(got["status"]))
    assert n == int(c["n_nodes"][i]), (name, n)
    assert n == len(q)
    dq = float(np.abs(got["robot_path"][:n] - q).max())
    assert dq <= q_tol, (name, dq)
    assert np.array_equal(got["robot_path"][0], c["q0"][i]) and np.array_equal(got["cube_path"][0], c["A"][i]), name
    ce = np.abs(got["cube_path"][:n] - cube).max(axis=1)
    bound = np.full(n, 1e-15) if not c["rotated"][i] else np.maximum(16 * err, 1e-15)
    assert (ce <= bound).all(), (name, ce.tolist(), bound.tolist())
    if tail_zero:
        assert not got["robot_path"][n:].any() and not got["cube_path"][n:].any(), name
    return dq, float((ce / bound).max())


def same(a, b, tol=SAME_TOL):
    """Two answers of one chain (chain_of), the row counts M possibly different:
    equal n_nodes and status, q within tol, cube rows bitwise equal."""
    n = int(a["n_nodes"])
    assert (n, int(a["status"])) == (int(b["n_nodes"]), int(b["status"]))
    assert np.abs(a["robot_path"][:n] - b["robot_path"][:n]).max() <= tol
    assert np.array_equal(a["cube_path"][:n], b["cube_path"][:n])


def run_alone(run, i, extra=2):
    c = cases()
    q0, A, B = inputs([i])
    return chain_of(run(q0, A, B, float(c["step_size"][i]), int(c["steps"][i]) + extra), 0)


def run_batch(run, which, idx, extra=2):
    q0, A, B = inputs(idx)
    return run(q0, A, B, step_size(which), longest(idx) + extra)


def check_max_nodes_edges(run):
    """On a reached chain of k steps, max_nodes = k + 1 gives status 0 and k + 1
    nodes (reached wins over cut), k gives status 3 and k nodes, a prefix of
    the former; max_nodes = 1 gives status 3, one node and row 0 = the inputs
    for every chain; the status-1 chain `obst` at max_nodes = its node count:
    status 3 and the same rows (cut wins over the stop the next step would find)."""
    c = cases()
    for name in ("path", "rz", "zero", "b4"):
        i = index(name)
        k = int(c["steps"][i])
        assert c["status"][i] == REACHED and c["n_nodes"][i] == k + 1
        q0, A, B = inputs([i])
        full = chain_of(run(q0, A, B, float(c["step_size"][i]), k + 1), 0)
        compare(i, full)
        cut = chain_of(run(q0, A, B, float(c["step_size"][i]), k), 0)
        assert (int(cut["n_nodes"]), int(cut["status"])) == (k, CUT), name
        assert np.array_equal(cut["robot_path"], full["robot_path"][:k]), name
        assert np.array_equal(cut["cube_path"], full["cube_path"][:k]), name
    for which in ("main", "boundary"):
        idx = group(which)
        q0, A, B = inputs(idx)
        one = run(q0, A, B, step_size(which), 1)
        assert (one["n_nodes"] == 1).all() and (one["status"] == CUT).all()
        assert np.array_equal(one["robot_path"][:, 0], q0) and np.array_equal(one["cube_path"][:, 0], A)
    i = index("obst")
    n = int(c["n_nodes"][i])
    assert c["status"][i] == COLLISION and n == 4
    q0, A, B = inputs([i])
    cut = chain_of(run(q0, A, B, float(c["step_size"][i]), n), 0)
    assert (int(cut["n_nodes"]), int(cut["status"])) == (n, CUT)
    full = run_alone(run, i)
    assert np.array_equal(cut["robot_path"], full["robot_path"][:n])
    assert np.array_equal(cut["cube_path"], full["cube_path"][:n])
