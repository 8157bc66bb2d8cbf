"""Planner-side callers of the IK: the reference's path.py
sampler and path projection, with every IK solve, collision check and
distance query batched on the GPU.

    q, placement = sample_cube_placement(robot, cube, cubeplacementq0, cubeplacementqgoal, viz=None)
    robot_path, cube_path = project_path(robot, cube, q_curr, cube_curr, cube_rand, step_size=0.025, viz=None)

Same names, arguments and results as /root/reference/path.py:27-62 and
:125-163.  `sample_cube_placement` draws its candidates from numpy's global
RandomState exactly as the reference does (x, y, z per attempt) but
evaluates them a batch at a time: cube-vs-environment check
(ikg_target_env_batch), cold-start IK with the collision term
(ikg_solve_batch), distanceToObstacle (ikg_distance_batch); the first valid
candidate in draw order is returned and the RandomState is left exactly
where the reference's sequential loop would leave it.  The reference's
progress prints are not reproduced; `viz` is shown once with the result.

Batched variants for planners that can use many samples / projections at
once: `sample_cube_placements` (n valid samples) and `project_paths` (many
warm-started projection chains advanced in lock-step, one batched solve per
step; `on_device=True` keeps the whole loop on the device, ikg_project_paths).

The planner itself (path.py:165-278):

    path = computepath(qinit, qgoal, cubeplacementq0, cubeplacementqgoal, robot=robot, cube=cube)
    paths = computepaths(robot, qinits, qgoals, cube_q0s, cube_goals, seeds)

`computepath` is the drop-in (numpy's global RandomState, the reference's draw
order); `computepaths` runs P planners in lock-step, each with its own
numpy Generator, the trees in device tensors.  Both drive `rrt_iteration`,
one RRT-Connect iteration whose nearest-neighbour query, projection and
connect distance are callables (the GPU's here, replayed ones in the CPU tests).

    report = checkpath(robot, path, per_segment=8)

checks what the planner does not: the straight joint-space segments between
the path's vertices, the connect jump included (ikg_trajectory_check_batch).
"""
from __future__ import annotations

import time

import numpy as np

from .config import DT_IK, EPSILON, MAX_ITERS
from .se3 import SE3, as_rt, interpolate, pack_targets
from .tools import setcubeplacement

MIN_OBSTACLE_DISTANCE = 0.04  # path.py:32
Z_RANGE = (1.05, 1.4)  # path.py:38


def _solver_scene(robot):
    solver = robot.solver
    if solver.scene is None:
        raise RuntimeError("the planner needs the robot's collision scene (ikgrasp.scene.setuppinocchio)")
    return solver, solver.scene


def _bounds(cubeplacementq0, cubeplacementqgoal):
    _, a = as_rt(cubeplacementq0)
    _, b = as_rt(cubeplacementqgoal)
    return ((min(a[0], b[0]), max(a[0], b[0])), (min(a[1], b[1]), max(a[1], b[1])), Z_RANGE)


def _rows(points):
    """placements [B,12] with identity rotation (path.py:48)."""
    out = np.zeros((points.shape[0], 12))
    out[:, [0, 4, 8]] = 1.0
    out[:, 9:] = points
    return out


def _evaluate(robot, placements, q0):
    """Candidates -> (valid [B] bool, q [B,nq]) per path.py:51-62."""
    solver, scene = _solver_scene(robot)
    B = placements.shape[0]
    valid = np.zeros(B, dtype=bool)
    q = np.zeros((B, solver.nq))
    free = np.nonzero(~solver.target_env(placements, scene.env_geoms()))[0]
    if free.size == 0:
        return valid, q
    sol = solver.solve(placements[free], q0, dtype="f64", eps=EPSILON, dt=DT_IK, max_iters=MAX_ITERS,
                       check_collision=True)
    ok = free[sol.converged.astype(bool)]
    q[free] = sol.q
    if ok.size:
        d = solver.distance(q[ok], placements[ok], scene.obstacle_pairs())
        valid[ok[d >= MIN_OBSTACLE_DISTANCE]] = True
    return valid, q


def sample_cube_placement(robot, cube, cubeplacementq0, cubeplacementqgoal, viz=None, batch=64):
    """path.py:27-62 (uniform sampler) -> (q, placement)."""
    (x0, x1), (y0, y1), (z0, z1) = _bounds(cubeplacementq0, cubeplacementqgoal)
    lo = np.array([x0, y0, z0])
    rng = np.array([x1 - x0, y1 - y0, z1 - z0])  # RandomState.uniform: low + (high - low) * u
    while True:
        state = np.random.get_state()
        u = np.random.random_sample((batch, 3))
        pts = lo + rng * u
        valid, q = _evaluate(robot, _rows(pts), robot.q0.copy())
        hit = np.nonzero(valid)[0]
        if hit.size == 0:
            continue  # the reference would have consumed the same 3 * batch draws
        i = int(hit[0])
        np.random.set_state(state)
        np.random.random_sample(3 * (i + 1))  # leave the stream where the sequential loop stops
        placement = SE3(np.eye(3), pts[i])
        setcubeplacement(robot, cube, placement)
        if viz is not None and hasattr(viz, "display"):
            viz.display(q[i])
        return q[i].copy(), placement


def sample_cube_placements(robot, cubeplacementq0, cubeplacementqgoal, n, rng=None, batch=1024):
    """n valid samples (q [n,nq], translations [n,3]) from a numpy Generator,
    evaluated `batch` candidates per round (no RandomState compatibility)."""
    rng = np.random.default_rng() if rng is None else rng
    (x0, x1), (y0, y1), (z0, z1) = _bounds(cubeplacementq0, cubeplacementqgoal)
    qs, ts = [], []
    while sum(len(t) for t in ts) < n:
        pts = np.stack([rng.uniform(x0, x1, batch), rng.uniform(y0, y1, batch), rng.uniform(z0, z1, batch)], 1)
        valid, q = _evaluate(robot, _rows(pts), robot.q0.copy())
        qs.append(q[valid])
        ts.append(pts[valid])
    return np.concatenate(qs)[:n], np.concatenate(ts)[:n]


def project_path(robot, cube, q_curr, cube_curr, cube_rand, step_size=0.025, viz=None):
    """path.py:125-163 -> (robot_path, cube_path), the valid prefix."""
    paths = project_paths(robot, [q_curr], [cube_curr], [cube_rand], step_size=step_size, cube=cube)
    if viz is not None and hasattr(viz, "display"):
        viz.display(paths[0][0][-1])
    return paths[0]


def _project_paths_device(robot, q_currs, cube_currs, cube_rands, step_size, cube):
    """project_paths through ikg_project_paths (host arrays in, lists out)."""
    solver, _ = _solver_scene(robot)
    C = len(q_currs)
    if C == 0:
        return []
    a, b = pack_targets(cube_currs), pack_targets(cube_rands)
    steps = [int(np.linalg.norm(a[c, 9:] - b[c, 9:]) / step_size) + 1 for c in range(C)]
    res = solver.project_paths(np.array(q_currs, dtype=np.float64), a, b, step_size=step_size,
                               max_nodes=max(steps) + 1, eps=EPSILON, dt=DT_IK, max_iters=MAX_ITERS)
    out = []
    for c in range(C):
        n = int(res["n_nodes"][c])
        rp = [np.array(q_currs[c], dtype=np.float64)] + [res["robot_path"][c, k].copy() for k in range(1, n)]
        cp = [cube_currs[c]] + [SE3(res["cube_path"][c, k, :9].reshape(3, 3), res["cube_path"][c, k, 9:])
                                for k in range(1, n)]
        out.append((rp, cp))
    if cube is not None and C == 1:  # the reference leaves the cube at the last attempt
        s = min(len(out[0][0]), steps[0])
        setcubeplacement(robot, cube, interpolate(SE3(*as_rt(cube_currs[0])), SE3(*as_rt(cube_rands[0])), s / steps[0]))
    return out


def project_paths(robot, q_currs, cube_currs, cube_rands, step_size=0.025, cube=None, on_device=False):
    """Many projections at once: chain c interpolates cube_currs[c] ->
    cube_rands[c] in int(|dt|/step_size)+1 steps (SE3.Interpolate), stops at
    the first cube/environment collision or failed IK, and warm-starts each
    solve from its previous q — the reference's loop per chain, with the
    active chains' step s solved in ONE batched launch.  Returns a list of
    (robot_path, cube_path).  on_device=True: the interpolation, the placement
    check and the bookkeeping run on the device too (ikg_project_paths), one
    call for the whole loop; the same list comes back."""
    if on_device:
        return _project_paths_device(robot, q_currs, cube_currs, cube_rands, step_size, cube)
    solver, scene = _solver_scene(robot)
    C = len(q_currs)
    env = scene.env_geoms()
    starts = [SE3(*as_rt(p)) for p in cube_currs]
    ends = [SE3(*as_rt(p)) for p in cube_rands]
    steps = [int(np.linalg.norm(a.translation - b.translation) / step_size) + 1 for a, b in zip(starts, ends)]
    robot_paths = [[np.array(q, dtype=np.float64)] for q in q_currs]
    cube_paths = [[p] for p in cube_currs]
    active = np.ones(C, dtype=bool)
    for s in range(1, max(steps) + 1):
        idx = [c for c in range(C) if active[c] and s <= steps[c]]
        if not idx:
            break
        pl = [interpolate(starts[c], ends[c], s / steps[c]) for c in idx]
        rows = np.stack([np.concatenate([p.rotation.reshape(9), p.translation]) for p in pl])
        col = solver.target_env(rows, env)
        go = [k for k in range(len(idx)) if not col[k]]
        for k in range(len(idx)):
            if col[k]:
                active[idx[k]] = False
        if cube is not None and C == 1:
            setcubeplacement(robot, cube, pl[-1])  # the reference leaves the cube at the last attempt, a colliding one too
        if not go:
            continue
        q0 = np.stack([robot_paths[idx[k]][-1] for k in go])
        sol = solver.solve(rows[go], q0, dtype="f64", eps=EPSILON, dt=DT_IK, max_iters=MAX_ITERS,
                           check_collision=True)
        for j, k in enumerate(go):
            c = idx[k]
            if not sol.converged[j]:
                active[c] = False
                continue
            robot_paths[c].append(sol.q[j].astype(np.float64))
            cube_paths[c].append(pl[k])
    return [(robot_paths[c], cube_paths[c]) for c in range(C)]


# ---------------------------------------------------------------- RRT-Connect (path.py:165-278)
START, GOAL = 0, 1
GOAL_BIAS = 0.1  # path.py:224


def displaypath(robot, path, dt, viz):
    """path.py:17-20."""
    for q in path:
        viz.display(q)
        time.sleep(dt)


def distance(q1, q2):
    """path.py:165-167."""
    return np.linalg.norm(q2 - q1)


def get_path(G):
    """path.py:176-184: the values from the root to the LAST vertex of G, a
    list of (parent index or None, value)."""
    path = []
    node = G[-1]
    while node[0] is not None:
        path.insert(0, node[1])
        node = G[node[0]]
    path.insert(0, G[0][1])
    return path


class Trees:
    """The start and goal trees of P planners: q[side] [P,cap,nq] and
    cube[side] [P,cap,12] (numpy arrays, or float64 tensors on `device`),
    with the vertex counts and the parent lists on the host.  Vertices are
    added as the reference adds them (add_edge_and_vertex): a projected
    segment whole, its first row -- the nearest vertex again -- included."""

    def __init__(self, qinits, qgoals, cube_q0s, cube_goals, cap=64, device=None):
        self.device = device
        roots_q = [np.asarray(qinits, dtype=np.float64), np.asarray(qgoals, dtype=np.float64)]
        roots_c = [pack_targets(cube_q0s), pack_targets(cube_goals)]
        self.P, self.nq = roots_q[0].shape
        self.cap = int(cap)
        self.q = [self._zeros(self.P, self.cap, self.nq) for _ in range(2)]
        self.cube = [self._zeros(self.P, self.cap, 12) for _ in range(2)]
        for side in (START, GOAL):
            self.q[side][:, 0] = self.asarray(roots_q[side])
            self.cube[side][:, 0] = self.asarray(roots_c[side])
        self.count = [np.ones(self.P, dtype=np.int64) for _ in range(2)]
        self.parents = [[[None] for _ in range(self.P)] for _ in range(2)]

    def _zeros(self, *shape):
        if self.device is None:
            return np.zeros(shape)
        import torch
        return torch.zeros(shape, dtype=torch.float64, device=self.device)

    def asarray(self, x):
        """A host array as the trees' kind of array."""
        if self.device is None:
            return np.asarray(x)
        import torch
        return torch.as_tensor(np.ascontiguousarray(x), device=self.device)

    def _index(self, x):
        return self.asarray(np.asarray(x, dtype=np.int64))

    def reset(self, p):
        """A retry of planner p: both trees back to their roots."""
        for side in (START, GOAL):
            self.count[side][p] = 1
            self.parents[side][p] = [None]

    def _grow(self, need):
        cap = self.cap
        while cap < need:
            cap *= 2
        for arrs, w in ((self.q, self.nq), (self.cube, 12)):
            for side in (START, GOAL):
                new = self._zeros(self.P, cap, w)
                new[:, :self.cap] = arrs[side]
                arrs[side] = new
        self.cap = cap

    def rows(self, side, planners, idx):
        """(q [A,nq], cube [A,12]) of vertex idx[a] of planner planners[a]."""
        pp, ii = self._index(planners), self._index(idx)
        return self.q[side][pp, ii], self.cube[side][pp, ii]

    def last(self, side, planners):
        return self.rows(side, planners, self.count[side][planners] - 1)

    def append(self, side, planners, near, seg_q, seg_cube, n):
        """Add rows 0 .. n[a]-1 of segment a to planner planners[a]'s tree:
        row 0 under vertex near[a], each later row under the one before."""
        n = np.asarray(n, dtype=np.int64)
        if int((self.count[side][planners] + n).max()) > self.cap:
            self._grow(int((self.count[side][planners] + n).max()))
        pp, rr, aa, jj = [], [], [], []
        for a, p in enumerate(planners):
            base = int(self.count[side][p])
            par = self.parents[side][p]
            for j in range(int(n[a])):
                par.append(base + j - 1 if j > 0 else int(near[a]))
                pp.append(p), rr.append(base + j), aa.append(a), jj.append(j)
            self.count[side][p] = base + int(n[a])
        pp, rr, aa, jj = (self._index(x) for x in (pp, rr, aa, jj))
        self.q[side][pp, rr] = seg_q[aa, jj]
        self.cube[side][pp, rr] = seg_cube[aa, jj]

    def _host(self, x):
        return x if self.device is None else x.cpu().numpy()

    def path(self, p):
        """path.py:264-267: root .. last start vertex, then last goal vertex .. root."""
        out = []
        for side in (START, GOAL):
            idx = get_path([(par, k) for k, par in enumerate(self.parents[side][p])])
            q = self._host(self.q[side][p][self._index(idx)])
            out.append([q[k].copy() for k in range(len(idx))])
        return out[START] + out[GOAL][::-1]

    def export(self, p):
        """Planner p's trees on the host: {start, goal}_{parent, q, cube};
        parent -1 = the root."""
        d = {}
        for side, name in ((START, "start"), (GOAL, "goal")):
            n = int(self.count[side][p])
            d[f"{name}_parent"] = np.array([-1 if x is None else x for x in self.parents[side][p]], dtype=np.int64)
            d[f"{name}_q"] = np.array(self._host(self.q[side][p, :n]))
            d[f"{name}_cube"] = np.array(self._host(self.cube[side][p, :n]))
        return d


def rrt_iteration(trees, planners, q_rand, cube_rand, nearest, project, connect):
    """One RRT-Connect iteration (path.py:231-262) of the listed planners.
    q_rand [A,nq], cube_rand [A,12]: each planner's sample (arrays of the
    trees' kind).  The three queries are callables:
      nearest(trees, side, planners, queries [A,nq]) -> vertex indices [A] (host ints)
      project(q_near [A,nq], cube_near [A,12], cube_to [A,12]) -> (seg_q [A,M,nq],
              seg_cube [A,M,12], n [A] host ints): project_path's valid prefixes
      connect(q_a [A,nq], q_b [A,nq]) -> |q_a - q_b| [A] (host floats)
    Returns (near_start [A], near_goal [A], connect distance [A])."""
    planners = list(planners)
    near0 = np.asarray(nearest(trees, START, planners, q_rand), dtype=np.int64)
    seg_q, seg_c, n = project(*trees.rows(START, planners, near0), cube_rand)
    trees.append(START, planners, near0, seg_q, seg_c, n)
    q_new, _ = trees.last(START, planners)
    near1 = np.asarray(nearest(trees, GOAL, planners, q_new), dtype=np.int64)
    _, goal_cube = trees.rows(GOAL, planners, np.zeros(len(planners), dtype=np.int64))  # cubeplacementqgoal
    seg_q, seg_c, n = project(*trees.rows(GOAL, planners, near1), goal_cube)
    trees.append(GOAL, planners, near1, seg_q, seg_c, n)
    q_end, _ = trees.last(GOAL, planners)
    return near0, near1, np.asarray(connect(q_new, q_end), dtype=np.float64)


def rrt_connect(trees, sample, nearest, project, connect, max_iterations=250, max_retries=10, goal_tolerance=0.5):
    """The planners of `trees` in lock-step until each has connected or run out
    of retries.  sample(planners) -> (q_rand [A,nq], cube_rand [A,12]) host
    arrays.  -> list of P paths ([] for a planner that failed; its trees are
    then those of its last retry)."""
    P = trees.P
    its, retries = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    done = np.zeros(P, dtype=bool) | (max_iterations <= 0) | (max_retries <= 0)
    paths = [[] for _ in range(P)]
    while not done.all():
        act = [p for p in range(P) if not done[p]]
        q_rand, cube_rand = sample(act)
        _, _, d = rrt_iteration(trees, act, trees.asarray(q_rand), trees.asarray(cube_rand), nearest, project, connect)
        for a, p in enumerate(act):
            if d[a] < goal_tolerance:
                paths[p] = trees.path(p)
                done[p] = True
                continue
            its[p] += 1
            if its[p] == max_iterations:
                its[p] = 0
                retries[p] += 1
                if retries[p] == max_retries:
                    done[p] = True
                else:
                    trees.reset(p)
    return paths


def _gpu_queries(robot, trees, step_size, max_nodes=None):
    """(nearest, project, connect) on the GPU for `trees` (host arrays: host
    pointers, each call returns its results; device tensors: device pointers,
    only the indices, counts and distances come back)."""
    solver, _ = _solver_scene(robot)
    host = trees.device is None
    to_host = (lambda x: np.asarray(x)) if host else (lambda x: x.cpu().numpy())

    def nearest(trees, side, planners, queries):
        counts = np.zeros(trees.P, dtype=np.int32)
        counts[planners] = trees.count[side][planners]
        full = trees._zeros(trees.P, trees.nq)
        full[trees._index(planners)] = queries
        idx, _ = solver.nearest(trees.q[side], trees.asarray(counts), full)
        return to_host(idx)[planners]

    def project(q_near, cube_near, cube_to):
        m = max_nodes
        if host:  # as many rows as the longest chain can fill
            m = int(np.max(np.linalg.norm(cube_near[:, 9:] - cube_to[:, 9:], axis=1) / step_size)) + 3
        res = solver.project_paths(q_near, cube_near, cube_to, step_size=step_size, max_nodes=m, eps=EPSILON,
                                   dt=DT_IK, max_iters=MAX_ITERS)
        status = to_host(res["status"])
        if (status == 3).any():
            raise RuntimeError("a projected segment was cut at max_nodes")
        return res["robot_path"], res["cube_path"], to_host(res["n_nodes"])

    def connect(q_a, q_b):
        A = q_a.shape[0]
        _, d = solver.nearest(q_b.reshape(A, 1, trees.nq), trees.asarray(np.ones(A, dtype=np.int32)), q_a)
        return to_host(d)

    return nearest, project, connect


def _segment_rows(cube_q0s, cube_goals, step_size):
    """Rows the longest projected segment of a query can have: every tree
    vertex lies in the box spanned by the two ends and the sampler's z range."""
    lo = np.array([np.inf] * 3)
    hi = -lo
    for a, b in zip(cube_q0s, cube_goals):
        for t in (as_rt(a)[1], as_rt(b)[1], np.array([as_rt(a)[1][0], as_rt(a)[1][1], Z_RANGE[0]]),
                  np.array([as_rt(b)[1][0], as_rt(b)[1][1], Z_RANGE[1]])):
            lo, hi = np.minimum(lo, t), np.maximum(hi, t)
    return int(np.linalg.norm(hi - lo) / step_size) + 3


def computepath(qinit, qgoal, cubeplacementq0, cubeplacementqgoal, robot=None, cube=None, *, max_iterations=250,
                max_retries=10, step_size=0.025, goal_tolerance=0.5, return_trees=False):
    """path.py:194-278 -> the list of configurations from qinit to qgoal, []
    when no path was found or `robot` / `cube` is missing.

    The reference's RRT-Connect with its constants, its draw order from numpy's
    global RandomState (`np.random.rand()` for the goal bias, then the sampler,
    which leaves the stream where the reference's would), its vertex
    bookkeeping and its connect test; both projections run through
    ikg_project_paths with one chain and the nearest-neighbour queries through
    ikg_nearest_batch.  Nothing is printed.

    Nearest neighbour: the lowest index among exact ties.  The reference's
    trees hold bitwise duplicates by construction (project_path returns its
    start vertex, which is added again), so scipy's KDTree tie-breaking decides
    how many repeated rows a returned path has; removing consecutive equal rows
    makes the path independent of that choice.

    return_trees=True: -> (path, Trees.export(0) of the last retry)."""
    if robot is None or cube is None:
        return ([], None) if return_trees else []
    trees = Trees([qinit], [qgoal], [cubeplacementq0], [cubeplacementqgoal])
    qgoal_row = np.asarray(qgoal, dtype=np.float64).reshape(1, -1)
    goal_row = pack_targets([cubeplacementqgoal])

    def sample(planners):
        if np.random.rand() < GOAL_BIAS:
            return qgoal_row, goal_row
        q, placement = sample_cube_placement(robot, cube, cubeplacementq0, cubeplacementqgoal, viz=None)
        return q.reshape(1, -1), pack_targets([placement])

    paths = rrt_connect(trees, sample, *_gpu_queries(robot, trees, step_size), max_iterations=max_iterations,
                        max_retries=max_retries, goal_tolerance=goal_tolerance)
    return (paths[0], trees.export(0)) if return_trees else paths[0]


def computepaths(robot, qinits, qgoals, cube_q0s, cube_goals, seeds, *, max_iterations=250, max_retries=10,
                 step_size=0.025, goal_tolerance=0.5, return_trees=False, batch=16, device=None):
    """P planners in lock-step -> list of P paths ([] for a planner that
    failed).  Planner p plans qinits[p] -> qgoals[p] with the cube from
    cube_q0s[p] to cube_goals[p], drawing from numpy.random.default_rng(seeds[p]):
    one number for the goal bias, then whole blocks of `batch` candidate
    placements until a block holds a valid one (the first in draw order is
    taken), so a planner's stream does not depend on which others run.

    Per iteration: one batched sampler round for the planners that need a
    sample, ikg_nearest_batch on the start trees, ikg_project_paths, nearest on
    the goal trees, project again, the connect test.  The trees live in device
    tensors [P,cap,nq] / [P,cap,12] with host-side parent lists; per iteration
    the samples go up and the nearest indices, segment counts, statuses and
    connect distances come back -- nothing that grows with the trees.
    Ties of the nearest neighbour go to the lowest index (see computepath).

    return_trees=True: -> (paths, [Trees.export(p)])."""
    import torch
    solver, _ = _solver_scene(robot)
    P = len(qinits)
    if P == 0:
        return ([], []) if return_trees else []
    dev = torch.device("cuda", solver.device) if device is None else torch.device(device)
    trees = Trees(qinits, qgoals, cube_q0s, cube_goals, device=dev)
    rngs = [np.random.default_rng(s) for s in seeds]
    goal_q, goal_c = np.asarray(qgoals, dtype=np.float64), pack_targets(cube_goals)
    bounds = [_bounds(a, b) for a, b in zip(cube_q0s, cube_goals)]
    lo = np.array([[b[k][0] for k in range(3)] for b in bounds])
    span = np.array([[b[k][1] - b[k][0] for k in range(3)] for b in bounds])
    q0 = robot.q0.copy()

    def sample(planners):
        q_rand, c_rand = goal_q[planners].copy(), goal_c[planners].copy()
        need = [a for a, p in enumerate(planners) if not rngs[p].random() < GOAL_BIAS]
        while need:  # one evaluation round for every planner still without a sample
            pts = np.concatenate([lo[planners[a]] + span[planners[a]] * rngs[planners[a]].random((batch, 3))
                                  for a in need])
            rows = _rows(pts)
            valid, q = _evaluate(robot, rows, q0)
            left = []
            for k, a in enumerate(need):
                hit = np.nonzero(valid[k * batch:(k + 1) * batch])[0]
                if hit.size:
                    q_rand[a], c_rand[a] = q[k * batch + hit[0]], rows[k * batch + hit[0]]
                else:
                    left.append(a)
            need = left
        return q_rand, c_rand

    rows = _segment_rows(cube_q0s, cube_goals, step_size)
    paths = rrt_connect(trees, sample, *_gpu_queries(robot, trees, step_size, max_nodes=rows),
                        max_iterations=max_iterations, max_retries=max_retries, goal_tolerance=goal_tolerance)
    return (paths, [trees.export(p) for p in range(P)]) if return_trees else paths


# ---------------------------------------------------------------- path check
def polyline_curves(path):
    """A path's straight segments as degree-2 Bezier curves -> (points
    [n_seg,3,nq], rows [n_seg+1,nq]).  Consecutive equal rows are dropped first;
    segment i has the control points q_i, (q_i + q_{i+1}) / 2, q_{i+1}, which is
    the straight line (a two-point curve is constant under the reference's
    Bezier semantics)."""
    rows = np.asarray(path, dtype=np.float64)
    if rows.ndim != 2 or len(rows) < 1:
        raise ValueError(f"a path is [n, nq], got {list(rows.shape)}")
    keep = np.ones(len(rows), dtype=bool)
    keep[1:] = np.any(rows[1:] != rows[:-1], axis=1)
    rows = rows[keep]
    a, b = rows[:-1], rows[1:]
    return np.stack([a, (a + b) / 2, b], axis=1), rows


def fold_segments(report, per_segment):
    """Per-segment reports with their per-sample arrays ([n_seg] and [n_seg,
    per_segment + 1], `IKSolver.check_curves(per_sample=True)`) -> one report of
    the whole path.  Sample k of segment i is path sample i * per_segment + k; a
    segment's last sample is the next one's first and is counted once, with the
    next segment (the last segment keeps its own).  Ties of an extreme go to the
    lowest path sample.  Adds `segment`, the segment of the first collision (-1
    = none), and `n_samples`."""
    ps = int(per_segment)
    col = np.asarray(report["collision"]).astype(bool)
    n_seg = col.shape[0]
    if n_seg == 0:
        raise ValueError("no segment to fold")
    own = np.ones((n_seg, ps + 1), dtype=bool)
    own[:-1, ps] = False

    def along(x):
        return np.asarray(x)[own]

    c = along(col)
    out = {"n_samples": int(c.size), "n_collision": int(c.sum()), "first_collision": -1, "first_pair": -1,
           "segment": -1}
    if c.any():
        k = int(np.argmax(c))
        seg = min(k // ps, n_seg - 1)
        out["first_collision"], out["segment"] = k, seg
        # the first colliding sample the fold sees in a segment is that segment's own first
        if int(np.asarray(report["first_collision"])[seg]) == k - seg * ps:
            out["first_pair"] = int(np.asarray(report["first_pair"])[seg])
    measured = bool(np.all(np.asarray(report["arg_clearance"]) >= 0))
    for name, key, pick in (("clearance", "min_clearance", np.argmin), ("grasp", "max_grasp", np.argmax),
                            ("limit", "max_limit", np.argmax)):
        x = along(report[name])
        k = int(pick(x))
        skip = name == "clearance" and not measured
        out[key] = float(x[k])
        out["arg_" + name] = -1 if skip else k
    for name in ("collision", "clearance", "grasp", "limit"):
        out[name] = along(report[name])
    return out


def checkpath(robot, path, per_segment=8, cube="carried", min_clearance=0.0, max_grasp=None, **kw):
    """A `computepath` result checked as the polyline the planner assumed, the
    connect jump included: every segment is sampled at per_segment + 1 points
    in one launch (`IKSolver.check_curves`) and the segments' reports are folded
    into one (`fold_segments`), sample indices counted along the path.  -> that
    report plus ok (`ikgrasp.control.trajectory_ok`).  `kw`: pair_idx,
    samples_per_wave."""
    from .control import trajectory_ok
    points, rows = polyline_curves(path)
    if len(points) == 0:
        raise ValueError("the path holds one configuration: nothing between vertices to check")
    rep = robot.solver.check_curves(points, 0.0, 1.0, samples=int(per_segment) + 1, cube=cube, per_sample=True, **kw)
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in rep.items()}
    out = fold_segments(host, per_segment)
    one = {k: np.asarray([out[k]]) for k in ("first_collision", "max_limit", "arg_clearance", "min_clearance",
                                             "max_grasp")}
    out["ok"] = bool(trajectory_ok(one, min_clearance, max_grasp)[0])
    return out
