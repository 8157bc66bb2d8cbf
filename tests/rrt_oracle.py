"""CPU ORACLE of the RRT-Connect planner — test infrastructure only.

`computepath` of the reference (path.py:194-278) restated over
oracle.planner_oracle (`sample_cube_placement`, `project_path`) with a numpy
RandomState standing for the reference's global np.random: the same draw
order (`rs.rand()` for the goal bias, then the sampler's x, y, z per attempt),
the same vertex bookkeeping (`add_edge_and_vertex`, `get_path`: every
projected segment is added whole, its first node -- the nearest vertex itself
-- included, so the trees hold bitwise duplicates), the same connect test.

Nearest neighbour: `nn="lowest"` takes the lowest index among exact ties
(the product's rule), `nn="kdtree"` asks scipy's KDTree as the reference does.
The two differ only in which of several equal rows is the parent, i.e. in how
many repeated rows a returned path has; `dedup` removes consecutive equal rows.

Every iteration is logged (bias flag, sample, nearest indices, both segments,
connect distance, the nearest-neighbour margins among distinct nodes) for the
fixtures of tests/golden/make_rrt_golden.py.
"""
from __future__ import annotations

import numpy as np

from oracle import planner_oracle as po


def get_path(G):
    """path.py:176-184."""
    path = []
    node = G[-1]
    while node[0] is not None:
        path.insert(0, node[1])
        node = G[node[0]]
    path.insert(0, G[0][1])
    return path


def dedup(path):
    """Remove consecutive bitwise-equal rows."""
    out = []
    for q in path:
        if not out or not np.array_equal(out[-1], q):
            out.append(q)
    return out


def nearest_lowest(points, target):
    """(index, distance, margin): least Euclidean distance, lowest index among
    exact ties; margin = distance gap to the nearest node with a different q
    (None when every node equals the winner)."""
    P = np.asarray(points)
    d2 = np.zeros(len(P))
    for j in range(P.shape[1]):  # the product's accumulation order
        d2 = d2 + (P[:, j] - target[j]) * (P[:, j] - target[j])
    i = int(np.argmin(d2))  # numpy: first occurrence of the minimum
    d = np.sqrt(d2)
    other = [k for k in range(len(P)) if not np.array_equal(P[k], P[i])]
    margin = float(d[other].min() - d[i]) if other else None
    return i, float(d[i]), margin


def nearest_kdtree(points, target):
    from scipy.spatial import KDTree
    d, i = KDTree(np.asarray(points)).query(target)
    _, _, margin = nearest_lowest(points, target)
    return int(i), float(d), margin


def computepath(scene, rs, qinit, qgoal, cube_q0, cube_goal, max_iterations=250, max_retries=10, step_size=0.025,
                goal_tolerance=0.5, nn="lowest"):
    """-> (path, trees, log).  cube_q0 / cube_goal are (R, t) pairs; path is []
    on failure; trees = the last retry's (G_start, G_cube_start, G_goal,
    G_cube_goal) lists of (parent, value); log = one dict per iteration."""
    nearest = {"lowest": nearest_lowest, "kdtree": nearest_kdtree}[nn]
    log = []
    trees = None
    for retry in range(max_retries):
        G_start, G_goal = [(None, qinit)], [(None, qgoal)]
        G_cube_start, G_cube_goal = [(None, cube_q0)], [(None, cube_goal)]
        trees = (G_start, G_cube_start, G_goal, G_cube_goal)
        for i in range(max_iterations):
            bias = bool(rs.rand() < 0.1)
            if bias:
                q_rand, cube_rand = qgoal, cube_goal
            else:
                q_rand, t, _ = po.sample_cube_placement(scene, rs, cube_q0[1], cube_goal[1])
                cube_rand = (np.eye(3), t)
            i0, _, m0 = nearest([g[1] for g in G_start], q_rand)
            seg_q, seg_c = po.project_path(scene, G_start[i0][1], G_cube_start[i0][1], cube_rand, step_size)
            for j in range(len(seg_q)):
                parent = len(G_start) - 1 if j > 0 else i0
                G_start.append((parent, seg_q[j]))
                G_cube_start.append((parent, seg_c[j]))
            q_new = seg_q[-1]
            i1, _, m1 = nearest([g[1] for g in G_goal], q_new)
            seg_qg, seg_cg = po.project_path(scene, G_goal[i1][1], G_cube_goal[i1][1], cube_goal, step_size)
            for j in range(len(seg_qg)):
                parent = len(G_goal) - 1 if j > 0 else i1
                G_goal.append((parent, seg_qg[j]))
                G_cube_goal.append((parent, seg_cg[j]))
            d = float(np.linalg.norm(seg_qg[-1] - q_new))
            log.append(dict(retry=retry, bias=bias, q_rand=np.array(q_rand), t_rand=np.array(cube_rand[1]),
                            near_start=i0, near_goal=i1, margin_start=m0, margin_goal=m1,
                            seg_start_q=np.array(seg_q), seg_start_t=np.array([c[1] for c in seg_c]),
                            seg_goal_q=np.array(seg_qg), seg_goal_t=np.array([c[1] for c in seg_cg]),
                            from_start_t=np.array(G_cube_start[i0][1][1]), from_goal_t=np.array(G_cube_goal[i1][1][1]),
                            connect=d))
            if d < goal_tolerance:
                return get_path(G_start) + get_path(G_goal)[::-1], trees, log
    return [], trees, log
