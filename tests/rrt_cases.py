"""Shared inputs of tests/test_rrt.py and tests/test_gpu_rrt.py (test infrastructure)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M_SEEDS = (3, 4, 6)

_cache = {}


def rrt_cases():
    if "rrt" not in _cache:
        _cache["rrt"] = dict(np.load(os.path.join(GOLDEN, "rrt_cases.npz")))
    return _cache["rrt"]


def rows12(t):
    """Identity-rotation placements [n,12] of translations [n,3]."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(t), 12))
    out[:, [0, 4, 8]] = 1.0
    out[:, 9:] = t
    return out


def dedup(path):
    """Remove consecutive bitwise-equal rows."""
    out = []
    for q in path:
        if not out or not np.array_equal(out[-1], q):
            out.append(np.asarray(q))
    return out


def nearest_reference(nodes, counts, queries):
    """numpy: least distance, the squared distance summed over j in order,
    first (lowest) index among exact ties; -1 for an empty tree."""
    P, _, nq = nodes.shape
    idx, dist = np.full(P, -1, dtype=np.int32), np.zeros(P)
    for p in range(P):
        n = int(counts[p])
        if n == 0:
            continue
        d2 = np.zeros(n)
        for j in range(nq):
            d = nodes[p, :n, j] - queries[p, j]
            d2 = d2 + d * d
        idx[p] = int(np.argmin(d2))
        dist[p] = np.sqrt(d2[idx[p]])
    return idx, dist


def nearest_cases():
    """[(name, nodes [P,cap,nq], counts [P], queries [P,nq])]: counts 1, 63, 64,
    65, 130 (one wave's lanes, one more, more than two rounds) at nq 1, 15, 32;
    P = 3 with unequal counts under a larger cap; the rows past each count hold
    the query itself (distance 0: must never win); bitwise-duplicate rows."""
    rng = np.random.default_rng(7)
    cases = []
    for nq in (1, 15, 32):
        for n in (1, 63, 64, 65, 130):
            cap = n + 3
            q = rng.normal(size=(1, nq))
            nodes = rng.normal(size=(1, cap, nq))
            nodes[0, n:] = q[0]
            cases.append((f"n{n}_nq{nq}", nodes, np.array([n], dtype=np.int32), q))
    counts = np.array([5, 130, 64], dtype=np.int32)
    q = rng.normal(size=(3, 15))
    nodes = rng.normal(size=(3, 200, 15))
    for p in range(3):
        nodes[p, counts[p]:] = q[p]
    cases.append(("P3_unequal", nodes, counts, q))
    # duplicates: the winner's row repeated at higher indices, in other lanes and in its own
    q = rng.normal(size=(2, 15))
    nodes = rng.normal(size=(2, 140, 15)) + 3.0
    counts = np.array([140, 70], dtype=np.int32)
    win = q + 0.01
    for p, rows in enumerate(([70, 6, 134, 71], [69, 5, 37])):
        for r in rows:
            nodes[p, r] = win[p]
    cases.append(("duplicates", nodes, counts, q))
    # a tree of nothing but copies of one row (the planner's first iterations)
    nodes = np.repeat(rng.normal(size=(1, 1, 15)), 9, axis=1)
    cases.append(("all_equal", nodes, np.array([9], dtype=np.int32), rng.normal(size=(1, 15))))
    cases.append(("empty", rng.normal(size=(2, 4, 15)), np.array([0, 2], dtype=np.int32), rng.normal(size=(2, 15))))
    return cases
