"""Controller kinematics on the GPU.

The reference controller (`/root/reference/control.py:242-410`, `controllaw`)
spends its kinematic work, per tick, in Pinocchio calls over the two hands:

    pin.computeAllTerms(model, data, q, vq); pin.updateFramePlacements      (:284-287)
    pin.computeJointJacobians / computeJointJacobiansTimeVariation          (:288-289)
    pin.forwardKinematics(model, data_des, q_des, vq_des)                   (:292-294)
    oMee = data.oMf[fid]; v_frame = pin.getFrameVelocity(..., LWA)          (:305-313)
    the same for the desired state                                          (:316-322)
    e = [x_des - x; log3(R_des R^T)], e_dot = v_des - v                     (:325-337)
    J = pin.computeFrameJacobian(..., LWA)                                   (:341-342)
    J_dot = pin.getFrameJacobianTimeVariation(..., LWA); J_dot @ vq          (:343-345)
    np.vstack / np.hstack over the two hands                                 (:368-371)

`task_space_terms` returns those stacked quantities for one state (the
drop-in for that block); `task_space_terms_batch` does many states in one
launch of `ikg_frame_kinematics_batch` (GPU).  `dynamics_terms_batch` gives
the dynamics of :284-286 (M from computeAllTerms, b from nonLinearEffects)
for many states in one launch of `ikg_dynamics_batch`, and
`control_torques_batch` the whole second half of the law (:284-406: the
operational-space inertia, the unconstrained QP and the torque line) through
`ikg_control_torque_batch`.  `controllaw` is the drop-in for the reference
function.  `maketraj` is the drop-in for the reference's trajectory fit
(control.py:63-197) and `maketraj_batch` fits B paths in one launch of
`ikg_bezier_fit_batch`; `save_trajectory` writes the reference's file.  `checktraj`
samples fitted curves for collision, clearance, grasp error and joint limits
in one launch of `ikg_trajectory_check_batch`; `dyntraj` answers whether the
motors can follow them (inverse dynamics and the URDF's velocity and effort
limits along the curve, `ikg_trajectory_dynamics_batch`) and `retime` stretches
them to the least duration that meets every limit.  `rollout` runs B closed loops of that law against a free-space
rigid-body plant in one call of `ikg_control_rollout` (desired state from the
Bezier curves, torque law, forward dynamics, semi-implicit Euler), and
`Simulation` is the same plant one tick at a time behind the simulator's
interface, so the reference's loop (control.py:461-463) runs without PyBullet.
Contact, the cube, joint limits and joint damping stay out of scope
(DESIGN.md §7).  There is no CPU path: without the HIP library these raise
`NativeLibraryError`.
"""
from __future__ import annotations

import json

import numpy as np

from . import _lib

WORLD, LOCAL, LOCAL_WORLD_ALIGNED = _lib.IKG_WORLD, _lib.IKG_LOCAL, _lib.IKG_LOCAL_WORLD_ALIGNED
HANDS = ("LARM_EFF", "RARM_EFF")  # control.py:273-276, row blocks 0-5 / 6-11


def frame_kinematics(robot, q, vq=None, rf=LOCAL_WORLD_ALIGNED, outputs=("placement", "velocity", "J", "dJ", "dJv"),
                     dtype="f64"):
    """Per-hand frame placement, velocity, Jacobian and its time variation
    in `rf` for a batch of states q, vq [B,nq] (GPU)."""
    return robot.solver.frame_kinematics(q, vq, rf=rf, outputs=outputs, dtype=dtype)


def task_space_terms_batch(robot, q, vq, q_des, vq_des, dtype="f64"):
    """control.py:284-345 for B states at once -> dict of
      J_total      [B,12,nq]  np.vstack of the hands' LOCAL_WORLD_ALIGNED Jacobians (:369)
      J_dot_v      [B,12]     J_dot @ vq per hand, stacked (:345, :370)
      e            [B,12]     [x_des - x; log3(R_des R^T)] per hand (:325-327, :335)
      e_dot        [B,12]     v_des - v per hand (:330-336)
      oMf          [B,2,12]   current hand placements (R row-major, t)
      v_frame      [B,2,6]    current hand velocities (LOCAL_WORLD_ALIGNED)."""
    r = robot.solver.frame_kinematics(q, vq, q_des, vq_des, rf=LOCAL_WORLD_ALIGNED,
                                      outputs=("placement", "velocity", "J", "dJv", "err", "derr"), dtype=dtype)
    return {"J_total": r["J"], "J_dot_v": r["dJv"], "e": r["err"], "e_dot": r["derr"], "oMf": r["placement"],
            "v_frame": r["velocity"]}


def task_space_terms(robot, q, vq, q_des, vq_des):
    """One controller tick's kinematic terms (control.py:284-345) ->
    (J_total [12,nq], J_dot_v_total [12], e [12], e_dot [12]), float64."""
    row = lambda x: np.asarray(x, dtype=np.float64).reshape(1, -1)
    r = task_space_terms_batch(robot, row(q), row(vq), row(q_des), row(vq_des))
    return r["J_total"][0], r["J_dot_v"][0], r["e"][0], r["e_dot"][0]


def dynamics_terms_batch(robot, q, vq=None, dtype="f64"):
    """control.py:284-286 for B states at once -> dict of
      M    [B,nq,nq]  robot.data.M after pin.computeAllTerms, both triangles filled
      b    [B,nq]     pin.nonLinearEffects(model, data, q, vq)
      g    [B,nq]     the gravity part of b (b at zero velocity)
    from one launch of `ikg_dynamics_batch` (GPU) with the body inertias of the
    robot's URDF (`ikgrasp.model.load_nextage_inertia`)."""
    r = robot.solver.dynamics(q, vq, outputs=("M", "nle", "g"), dtype=dtype)
    return {"M": r["M"], "b": r["nle"], "g": r["g"]}


def control_torques_batch(robot, q, vq, q_des, vq_des, **gains):
    """control.py:284-406 for B states at once (GPU, fp64) -> dict of
      tau [B,nq], q_ddot_desired [B,nq], x_ddot_des_total [B,12], Lambda [B,2,6,6], f_c_total [B,12]
    (f_c_total before the :375 bias, which enters tau only).  `gains`: Kp, Kv,
    Kf, Kt, lambda_reg, qp_reg, fc_bias, zero_tau; defaults are the reference's."""
    r = robot.solver.control_torques(q, vq, q_des, vq_des, **gains)
    return {"tau": r["tau"], "q_ddot_desired": r["qdd"], "x_ddot_des_total": r["xdd"],
            "Lambda": r["Lambda"].reshape(-1, 2, 6, 6), "f_c_total": r["fc"]}


def controllaw(sim, robot, trajs, tcurrent, cube):
    """Drop-in for the reference's `controllaw(sim, robot, trajs, tcurrent, cube)`
    (control.py:242-410): reads the simulator state, evaluates the desired
    trajectory at tcurrent, computes the torques in one B = 1 call of
    `ikg_control_torque_batch` and steps the simulator with them."""
    q, vq = sim.getpybulletstate()  # :254
    row = lambda x: np.asarray(x, dtype=np.float64).reshape(1, -1)
    q_des, vq_des = trajs[0](tcurrent), trajs[1](tcurrent)  # :269-270
    tau = robot.solver.control_torques(row(q), row(vq), row(q_des), row(vq_des), outputs=("tau",))["tau"][0]
    sim.step(tau.tolist())  # :410


# ---------------------------------------------------------------- closed loop (control.py:415-463)
class Curve:
    """A Bezier curve with the reference class's attributes (control_points_,
    T_min_, T_max_, mult_T_) and call semantics (control.py:18-46).  Calling it
    evaluates ONE time on the host, for the per-tick drop-in `controllaw`;
    batches go through `IKSolver.bezier` / `rollout`."""

    def __init__(self, pointlist, t_min=0.0, t_max=1.0, mult_t=1.0):
        self.control_points_ = [np.asarray(p, dtype=np.float64) for p in pointlist]
        self.T_min_, self.T_max_, self.mult_T_ = float(t_min), float(t_max), float(mult_t)
        self.degree_ = len(self.control_points_) - 1
        if self.degree_ < 1 or self.T_max_ <= self.T_min_:
            raise ValueError("a curve needs two control points and t_max > t_min")

    def __call__(self, t):
        if not (self.T_min_ <= t <= self.T_max_):
            raise ValueError("time out of the curve's range")
        P = self.control_points_
        if self.degree_ == 1:
            return self.mult_T_ * P[0]
        u = (t - self.T_min_) / (self.T_max_ - self.T_min_)
        uo, bc, tn = 1.0 - u, 1.0, 1.0
        tmp = P[0] * uo
        for i in range(1, self.degree_):
            tn *= u
            bc *= (self.degree_ - i + 1) / i
            tmp = (tmp + (tn * bc) * P[i]) * uo
        return (tmp + (tn * u) * P[-1]) * self.mult_T_

    def derivative(self, order=1):
        """Bezier.derivative: control points degree (P[i+1] - P[i]), mult * (1 / (t_max - t_min))."""
        c = self
        for _ in range(order):
            P = c.control_points_
            pts = [c.degree_ * (b - a) for a, b in zip(P[:-1], P[1:])]
            if len(pts) < 2:
                pts = pts + pts  # a constant: two equal points evaluate to mult P0
            c = Curve(pts, c.T_min_, c.T_max_, c.mult_T_ * (1.0 / (c.T_max_ - c.T_min_)))
        return c


def load_trajectory(path):
    """The reference's trajectory file (save_trajectory_to_json: q_, vq_,
    vvq_control_points, t_min, t_max, mult_t) -> (q_of_t, vq_of_t, vvq_of_t).
    As load_trajectory_from_json does, EVERY curve gets the file's mult_t, so a
    file-loaded velocity curve is the unscaled derivative (the 1 / (t_max -
    t_min) of Bezier.derivative is not stored); `q_of_t.derivative(1)` gives the
    scaled one."""
    with open(path) as f:
        d = json.load(f)
    return tuple(Curve(d[k], d["t_min"], d["t_max"], d["mult_t"])
                 for k in ("q_control_points", "vq_control_points", "vvq_control_points"))


def save_trajectory(path, trajs):
    """The reference's save_trajectory_to_json (control.py:203-215): the three
    curves' control points and the q curve's t_min, t_max, mult_t.  The file
    does not store the derivatives' multipliers, so `load_trajectory` gives
    every curve the file's mult_t (its documented quirk)."""
    q_of_t, vq_of_t, vvq_of_t = trajs
    pts = lambda c: [np.asarray(p, dtype=np.float64).tolist() for p in c.control_points_]
    with open(path, "w") as f:
        json.dump({"q_control_points": pts(q_of_t), "vq_control_points": pts(vq_of_t),
                   "vvq_control_points": pts(vvq_of_t), "t_min": q_of_t.T_min_, "t_max": q_of_t.T_max_,
                   "mult_t": q_of_t.mult_T_}, f, indent=4)


FIT_MAX_POINTS = 256  # ikg_bezier_fit_batch: path points per path
FLAG_COST = 0.15      # control.py:191: `result.fun < 0.15`


class FittedTrajectories:
    """B fitted trajectories (`maketraj_batch`): points [B,degree+1,nq],
    vpoints [B,degree,nq] and apoints [B,degree-1,nq] (the unscaled derivative
    control points), cost [B], ok [B] = cost < 0.15 (the reference's flag),
    t_min = 0 and t_max = total_time.  `curves(i)` is path i's (q_of_t,
    vq_of_t, vvq_of_t); `rollout` takes the object as `trajs`."""

    def __init__(self, points, vpoints, apoints, cost, total_time):
        self.points, self.vpoints, self.apoints, self.cost = points, vpoints, apoints, cost
        self.ok = cost < FLAG_COST
        self.t_min, self.t_max = 0.0, float(total_time)

    def __len__(self):
        return len(self.points)

    def curves(self, i):
        q_of_t = Curve(list(self.points[i]), self.t_min, self.t_max)
        return q_of_t, q_of_t.derivative(1), q_of_t.derivative(2)

    def check(self, robot, **kw):
        """`checktraj(robot, self, **kw)`: one verdict per fitted curve."""
        return checktraj(robot, self, **kw)

    def dynamics(self, robot, **kw):
        """`dyntraj(robot, self, **kw)`: the actuator-limit report of every fitted curve."""
        return dyntraj(robot, self, **kw)


def maketraj_batch(q0s, q1s, paths, total_time, degree=20, ridge=None, solver=None):
    """The reference's maketraj (control.py:63-197) for B paths in one launch of
    `ikg_bezier_fit_batch` (GPU, fp64).  The reference's six equality
    constraints pin three control points at each end; the remaining degree - 5
    are a linear least-squares problem, which the kernel solves exactly
    (SLSQP with finite-difference gradients stops early: the cost here is never
    above the reference's).  q0s, q1s [B,nq]; paths: B arrays [n_i, nq],
    2 <= n_i <= 256, packed here on the host.
    ridge=None: 0 when every path has n >= degree - 3 points (the reference's
    problem, 17 at degree 20), else 1e-10: a shorter path leaves the
    reference's problem underdetermined and the ridge term picks the solution
    nearest its initial guess linspace(q0, q1).  A ridge > 0 also damps the
    large control polygons an exact fit of a noisy path produces.
    `solver`: whose `bezier_fit` runs (an IKSolver: its device); default device 0.
    -> FittedTrajectories."""
    from . import solver as _solver
    paths = [np.asarray(p, dtype=np.float64) for p in paths]
    q0s = np.asarray(q0s, dtype=np.float64)
    q0s = q0s.reshape(len(paths), -1)
    nq = q0s.shape[1]
    for i, p in enumerate(paths):
        if p.ndim != 2 or p.shape[1] != nq:
            raise ValueError(f"path {i} must be [n, {nq}], got {list(p.shape)}")
        if not 2 <= len(p) <= FIT_MAX_POINTS:
            raise ValueError(f"path {i} has {len(p)} points (2 .. {FIT_MAX_POINTS})")
    if ridge is None:
        ridge = 0.0 if all(len(p) >= degree - 3 for p in paths) else 1e-10
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    packed = np.concatenate(paths) if paths else np.zeros((0, nq))
    fit = solver.bezier_fit if solver is not None else _solver.bezier_fit
    r = fit(q0s, q1s, packed, offsets, total_time=total_time, degree=degree, ridge=ridge)
    return FittedTrajectories(r["points"], r["vpoints"], r["apoints"], r["cost"], total_time)


def maketraj(q0, q1, path_points, total_time, ridge=None, solver=None):
    """Drop-in for the reference's `maketraj(q0, q1, path_points, total_time)`
    (control.py:63-197) -> ([q_of_t, vq_of_t, vvq_of_t], flag): the degree-20
    curve through `maketraj_batch` with B = 1, its derivatives exactly
    q_of_t.derivative(1) and .derivative(2), flag = cost < 0.15 (:191).
    ridge=None: 0 for 17 points or more, 1e-10 below (see maketraj_batch).
    More than 256 points raise ValueError.  The reference's prints and its
    trajectory2.json side effect are not reproduced (`save_trajectory`)."""
    fitted = maketraj_batch([q0], [q1], [path_points], total_time, degree=20, ridge=ridge, solver=solver)
    return list(fitted.curves(0)), bool(fitted.ok[0])


def trajectory_ok(report, min_clearance=0.0, max_grasp=None):
    """The verdict of a trajectory-check report (numpy arrays [B]): no colliding
    sample, every sample inside the joint limits, the clearance to the obstacle
    pairs never below `min_clearance` (where a clearance was computed:
    arg_clearance >= 0) and, when `max_grasp` is given, the grasp error never
    above it -> bool [B]."""
    ok = (np.asarray(report["first_collision"]) < 0) & (np.asarray(report["max_limit"]) == 0.0)
    measured = np.asarray(report["arg_clearance"]) >= 0
    ok &= ~measured | (np.asarray(report["min_clearance"]) >= min_clearance)
    if max_grasp is not None:
        ok &= np.asarray(report["max_grasp"]) <= max_grasp
    return ok


def checktraj(robot, trajs, samples=151, cube="carried", min_clearance=0.0, max_grasp=None, per_sample=False, **kw):
    """What the planner checks at its vertices only, along whole curves: each
    curve is sampled at `samples` times in one launch of
    `ikg_trajectory_check_batch` (GPU, fp64) for collision (the cube carried by
    the left hand, or at fixed placements), clearance to the obstacle pairs,
    the grasp error the IK compares with EPSILON and the joint limits.
    trajs: one (q_of_t, vq_of_t, vvq_of_t) tuple as `maketraj` returns, a
    `Curve`, or a `FittedTrajectories`.  -> the report of
    `IKSolver.check_curves` plus ok [B] (`trajectory_ok`).  `kw`: pair_idx,
    samples_per_wave."""
    if isinstance(trajs, FittedTrajectories):
        points, t_min, t_max, mult = np.asarray(trajs.points, dtype=np.float64), trajs.t_min, trajs.t_max, 1.0
    else:
        q_of_t = trajs if hasattr(trajs, "control_points_") else trajs[0]
        pts, t_min, t_max, mult = _lib.curve(q_of_t)
        points = pts[None]
    report = robot.solver.check_curves(points, t_min, t_max, mult=mult, samples=samples, cube=cube,
                                       per_sample=per_sample, **kw)
    report["ok"] = trajectory_ok(report, min_clearance, max_grasp)
    return report


def _curve_set(trajs):
    """trajs as `checktraj` takes them -> (points [B,n,nq], t_min, t_max, mult)"""
    if isinstance(trajs, FittedTrajectories):
        return np.asarray(trajs.points, dtype=np.float64), trajs.t_min, trajs.t_max, 1.0
    q_of_t = trajs if hasattr(trajs, "control_points_") else trajs[0]
    pts, t_min, t_max, mult = _lib.curve(q_of_t)
    return pts[None], t_min, t_max, mult


def dyntraj(robot, trajs, samples=151, velocity=None, effort=None, per_sample=False, **kw):
    """Can the motors follow these curves in their duration, and if not how
    long must they take?  Each curve is sampled at `samples` times (the times
    of `checktraj`) in one launch of `ikg_trajectory_dynamics_batch` (GPU,
    fp64): joint velocity and acceleration from the curve's derivatives, the
    joint torques by recursive Newton-Euler, and their ratios to the limits.
    trajs: as `checktraj`.  velocity, effort: the joints' limits; None = the
    robot's (`robot.actuation`, the URDF's <limit velocity effort>), unlimited
    for a robot without them.  -> the report of `IKSolver.curve_dynamics` plus
    ok [B] = n_static == 0 and speed_scale <= 1 and torque_use <= 1, and
    least_duration [B] = (t_max - t_min) max(speed_scale, torque_scale), the
    shortest duration of the same curve that meets every limit (inf where
    n_static > 0: a joint cannot hold the posture at any speed).  `kw`:
    samples_per_wave."""
    points, t_min, t_max, mult = _curve_set(trajs)
    act = getattr(robot, "actuation", None)
    if velocity is None and act is not None:
        velocity = act.velocity
    if effort is None and act is not None:
        effort = act.effort
    report = robot.solver.curve_dynamics(points, t_min, t_max, mult=mult, samples=samples, velocity=velocity,
                                         effort=effort, per_sample=per_sample, **kw)
    static = np.asarray(report["n_static"]) > 0
    report["ok"] = ~static & (np.asarray(report["speed_scale"]) <= 1.0) & (np.asarray(report["torque_use"]) <= 1.0)
    scale = np.maximum(np.asarray(report["speed_scale"]), np.asarray(report["torque_scale"]))
    report["least_duration"] = np.where(static, np.inf, (float(t_max) - float(t_min)) * scale)
    return report


def retime(robot, trajs, margin=1.0, **kw):
    """The same curve(s) at the least duration that meets every actuator limit
    (`dyntraj`'s least_duration) times `margin`: uniform time scaling moves
    t_max only, so nothing is fitted again.  One trajectory (a tuple as
    `maketraj` returns, or a `Curve`) -> [q_of_t, vq_of_t, vvq_of_t] with
    t_max = t_min + margin least_duration and the derivative curves rebuilt
    from the new range.  A `FittedTrajectories` -> (durations [B] = margin
    least_duration, a `FittedTrajectories` of the same control points whose
    total_time is the largest of them: the shortest common duration at which
    every curve is feasible).  ValueError where n_static > 0.  `kw`: dyntraj's."""
    report = dyntraj(robot, trajs, **kw)
    if (np.asarray(report["n_static"]) > 0).any():
        bad = np.flatnonzero(np.asarray(report["n_static"]) > 0).tolist()
        raise ValueError(f"curves {bad}: gravity alone exceeds an effort limit (n_static > 0), no duration is feasible")
    durations = float(margin) * np.asarray(report["least_duration"], dtype=np.float64)
    if not (durations > 0).all():
        raise ValueError("a curve that does not move has no least duration")
    if isinstance(trajs, FittedTrajectories):
        return durations, FittedTrajectories(trajs.points, trajs.vpoints, trajs.apoints, trajs.cost,
                                             float(durations.max()))
    q_of_t = trajs if hasattr(trajs, "control_points_") else trajs[0]
    q_new = Curve(q_of_t.control_points_, q_of_t.T_min_, q_of_t.T_min_ + float(durations[0]), q_of_t.mult_T_)
    return [q_new, q_new.derivative(1), q_new.derivative(2)]


def rollout(robot, q0, vq0, trajs, t0=None, ticks=1500, **kw):
    """B closed loops of `controllaw` against the free rigid-body plant in one
    call (`IKSolver.rollout`, GPU, fp64): trajs = (q_of_t, vq_of_t[, ...]) as
    the reference passes them; dt_sim, dt_traj, record_every, outputs and the
    gains as keywords.  1,500 ticks are the reference's 15 s run.
    One trajectory per state (`ikg_control_rollout_curves`): trajs = a
    `FittedTrajectories`, or (points [B,n,nq], vpoints [B,n-1,nq], t_min,
    t_max) with the unscaled derivative points; the v curves get
    Bezier.derivative's multiplier 1 / (t_max - t_min)."""
    if isinstance(trajs, FittedTrajectories):
        trajs = (trajs.points, trajs.vpoints, trajs.t_min, trajs.t_max)
    if len(trajs) == 4 and getattr(trajs[0], "ndim", 0) == 3:
        points, vpoints, t_min, t_max = trajs
        t_min, t_max = float(t_min), float(t_max)
        sets = ((points, t_min, t_max, 1.0), (vpoints, t_min, t_max, 1.0 * (1.0 / (t_max - t_min))))
        return robot.solver.rollout(q0, vq0, sets, t0=t0, ticks=ticks, per_state=True, **kw)
    return robot.solver.rollout(q0, vq0, (trajs[0], trajs[1]), t0=t0, ticks=ticks, **kw)


class Simulation:
    """The simulator's interface (getpybulletstate / setqsim / step) over the
    free rigid-body plant: `step(torques)` is one B = 1 call of
    `ikg_forward_dynamics_batch` and a semi-implicit Euler update (v += dt qdd,
    q += dt v: Bullet's scheme), so the reference's loop
        while tcur < total_time: controllaw(sim, robot, trajs, tcur, cube); tcur += DT
    runs unmodified.  No contact, cube, joint limits or damping."""

    def __init__(self, robot, dt=1e-3):
        self.solver = robot.solver if hasattr(robot, "solver") else robot
        self.dt = float(dt)
        self.q = np.zeros(self.solver.nq)
        self.v = np.zeros(self.solver.nq)

    def setqsim(self, q, v=None):
        self.q = np.array(q, dtype=np.float64).reshape(-1)
        self.v = np.zeros_like(self.q) if v is None else np.array(v, dtype=np.float64).reshape(-1)

    def getpybulletstate(self):
        return self.q.copy(), self.v.copy()

    def step(self, torques):
        tau = np.asarray(torques, dtype=np.float64).reshape(1, -1)
        qdd = self.solver.forward_dynamics(self.q.reshape(1, -1), self.v.reshape(1, -1), tau)[0]
        self.v = self.v + self.dt * qdd
        self.q = self.q + self.dt * self.v
