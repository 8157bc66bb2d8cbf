"""CPU ORACLE -- test infrastructure only, never the product path.

Independent restatement of the controller's dynamics and torque law
(reference control.py:284-410) in Pinocchio's formulation: spatial algebra in
BODY-LOCAL coordinates over the joint tree (the HIP kernel works in one world
frame, csrc/ikg_dynamics.hpp, so the two derivations share nothing):

  pin.rnea / pin.nonLinearEffects   v_i = liMi.actInv(v_p) + S_i qd_i
                                    a_i = liMi.actInv(a_p) + S_i qdd_i + v_i x S_i qd_i,  a_universe = -gravity
                                    f_i = Y_i a_i + v_i x* (Y_i v_i);  tau_i = S_i . f_i;  f_p += liMi.act(f_i)
  pin.crba / computeAllTerms        Ycrb_i = Y_i + sum_children liMi.act(Ycrb_c);  F = Ycrb_i S_i, carried up
                                    the support chain with liMi.act:  M[i,j] = M[j,i] = S_j . F
  control.py:284-410                `controllaw_terms`, line by line, with inv / solve where the reference
                                    has np.linalg.inv / quadprog.solve_qp (no constraints: H^-1 d)

Motions are [linear; angular], SE3 = (R, p), the conventions of
oracle/control_oracle.py.  The model is a `DualArmModel` (canonical-axis joint
tables) with `BodyInertias`.

Every function takes an arithmetic `ar`: F64 (numpy float64), F32 (every
operation rounded to float32: the measured fp32 bound of M / nle / g) or
MP (mpmath at 50 digits: the truth the controller outputs are measured
against).  Arrays are numpy arrays of ar.dtype (object arrays of mpf for MP).
"""
from __future__ import annotations

import math

import numpy as np

GRAVITY = (0.0, 0.0, -9.81)


class F64:
    dtype = np.float64
    num = staticmethod(float)
    sin, cos, sqrt, acos = (staticmethod(f) for f in (math.sin, math.cos, math.sqrt, math.acos))

    @staticmethod
    def inv(A):
        return np.linalg.inv(A)

    @staticmethod
    def solve(A, b):
        return np.linalg.solve(A, b)


class F32:
    dtype = np.float32
    num = staticmethod(np.float32)
    sin = staticmethod(lambda x: np.float32(np.sin(np.float32(x))))
    cos = staticmethod(lambda x: np.float32(np.cos(np.float32(x))))
    sqrt = staticmethod(lambda x: np.float32(np.sqrt(np.float32(x))))


class MP:
    """mpmath, 50 significant digits."""
    dtype = object
    DPS = 50

    @staticmethod
    def _mp():
        import mpmath
        mpmath.mp.dps = MP.DPS
        return mpmath

    @staticmethod
    def num(x):
        return MP._mp().mpf(float(x)) if not hasattr(x, "_mpf_") else x

    sin = staticmethod(lambda x: MP._mp().sin(x))
    cos = staticmethod(lambda x: MP._mp().cos(x))
    sqrt = staticmethod(lambda x: MP._mp().sqrt(x))
    acos = staticmethod(lambda x: MP._mp().acos(x))

    @staticmethod
    def inv(A):
        mp = MP._mp()
        return np.array(mp.inverse(mp.matrix(A.tolist())).tolist(), dtype=object)

    @staticmethod
    def solve(A, b):
        mp = MP._mp()
        x = mp.lu_solve(mp.matrix(A.tolist()), mp.matrix(list(b)))
        return np.array([x[i] for i in range(len(b))], dtype=object)


def arr(ar, x):
    """array of the arithmetic's numbers from floats"""
    a = np.asarray(x, dtype=np.float64)
    if ar.dtype is object:
        out = np.empty(a.shape, dtype=object)
        for idx in np.ndindex(a.shape):
            out[idx] = ar.num(a[idx])
        return out
    return a.astype(ar.dtype)


def to_f64(x):
    return np.array([float(t) for t in np.asarray(x).reshape(-1)], dtype=np.float64).reshape(np.shape(x))


def zeros(ar, *shape):
    return arr(ar, np.zeros(shape))


def eye(ar, n):
    return arr(ar, np.eye(n))


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=a.dtype)


def skew(ar, p):
    z = ar.num(0.0)
    return np.array([[z, -p[2], p[1]], [p[2], z, -p[0]], [-p[1], p[0], z]], dtype=ar.dtype)


def axis_rotation(ar, axis, q):
    """JointModelR{X,Y,Z}: the rotation about canonical axis 0/1/2."""
    s, c = ar.sin(q), ar.cos(q)
    R = eye(ar, 3)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


# ---------------------------------------------------------------- SE3 actions (6x6 forms)
def motion_matrix(ar, M):
    """SE3.act on motions [v; w]: [[R, [p]x R], [0, R]]."""
    R, p = M
    X = zeros(ar, 6, 6)
    X[:3, :3], X[:3, 3:], X[3:, 3:] = R, skew(ar, p) @ R, R
    return X


def force_matrix(ar, M):
    """SE3.act on forces [f; n]: [[R, 0], [[p]x R, R]]."""
    R, p = M
    X = zeros(ar, 6, 6)
    X[:3, :3], X[3:, :3], X[3:, 3:] = R, skew(ar, p) @ R, R
    return X


def se3_inv(M):
    R, p = M
    return R.T, -(R.T @ p)


def spatial_inertia(ar, mass, com, I_com):
    """Inertia (m, c, I_c) as the 6x6 map motion -> force:
    [[m 1, -m [c]x], [m [c]x, I_c - m [c]x [c]x]]."""
    m = ar.num(mass)
    C = skew(ar, arr(ar, com))
    Y = zeros(ar, 6, 6)
    Y[:3, :3] = m * eye(ar, 3)
    Y[:3, 3:] = -(m * C)
    Y[3:, :3] = m * C
    Y[3:, 3:] = arr(ar, I_com) - m * (C @ C)
    return Y


def motion_cross(a, b):
    return np.concatenate([cross(a[3:], b[:3]) + cross(a[:3], b[3:]), cross(a[3:], b[3:])])


def force_cross(v, f):
    """v x* f = [w x f; w x n + v x f]."""
    return np.concatenate([cross(v[3:], f[:3]), cross(v[3:], f[3:]) + cross(v[:3], f[:3])])


class Tree:
    """The model in one arithmetic: placements, axes, parents, body inertias."""

    def __init__(self, ar, model, inertias, gravity=GRAVITY):
        self.ar, self.nq = ar, model.nq
        self.parent = [int(p) for p in model.parents]
        self.axis = [int(a) for a in model.axis]
        self.R0 = [arr(ar, model.R[j]) for j in range(model.nq)]
        self.t0 = [arr(ar, model.t[j]) for j in range(model.nq)]
        Im = inertias.matrices()
        self.Y = [spatial_inertia(ar, inertias.mass[j], inertias.com[j], Im[j]) for j in range(model.nq)]
        self.S = []
        for j in range(model.nq):
            s = zeros(ar, 6)
            s[3 + self.axis[j]] = ar.num(1.0)
            self.S.append(s)
        self.gravity = arr(ar, gravity)
        self.hand = [(arr(ar, model.hand_R[h]), arr(ar, model.hand_t[h])) for h in range(2)]
        self.hand_joint = [int(model.arm_q[h][-1]) for h in range(2)]

    def liMi(self, q):
        return [(self.R0[j] @ axis_rotation(self.ar, self.axis[j], q[j]), self.t0[j]) for j in range(self.nq)]


def rnea(tree, q, v, a):
    """pin.rnea(model, data, q, v, a): the joint torques."""
    ar, nq = tree.ar, tree.nq
    q, v, a = arr(ar, q), arr(ar, v), arr(ar, a)
    li = tree.liMi(q)
    a0 = np.concatenate([-tree.gravity, zeros(ar, 3)])
    vs, acc, f = [], [], []
    for i in range(nq):
        Xinv = motion_matrix(ar, se3_inv(li[i]))
        p = tree.parent[i]
        vi = tree.S[i] * v[i] + (Xinv @ vs[p] if p >= 0 else zeros(ar, 6))
        ai = tree.S[i] * a[i] + motion_cross(vi, tree.S[i] * v[i]) + Xinv @ (acc[p] if p >= 0 else a0)
        vs.append(vi)
        acc.append(ai)
        f.append(tree.Y[i] @ ai + force_cross(vi, tree.Y[i] @ vi))
    tau = zeros(ar, nq)
    for i in reversed(range(nq)):
        tau[i] = tree.S[i] @ f[i]
        if tree.parent[i] >= 0:
            f[tree.parent[i]] = f[tree.parent[i]] + force_matrix(ar, li[i]) @ f[i]
    return tau


def nle(tree, q, v):
    """pin.nonLinearEffects = rnea(q, v, 0)."""
    return rnea(tree, q, v, np.zeros(tree.nq))


def gravity_torques(tree, q):
    """pin.computeGeneralizedGravity = rnea(q, 0, 0)."""
    return rnea(tree, q, np.zeros(tree.nq), np.zeros(tree.nq))


def crba(tree, q):
    """pin.crba with the lower triangle filled (data.M as control.py uses it)."""
    ar, nq = tree.ar, tree.nq
    li = tree.liMi(arr(ar, q))
    Yc = [y.copy() for y in tree.Y]
    M = zeros(ar, nq, nq)
    for i in reversed(range(nq)):
        F = Yc[i] @ tree.S[i]
        M[i, i] = tree.S[i] @ F
        j = i
        while tree.parent[j] >= 0:
            F = force_matrix(ar, li[j]) @ F
            j = tree.parent[j]
            M[i, j] = M[j, i] = tree.S[j] @ F
        if tree.parent[i] >= 0:
            X = force_matrix(ar, li[i])
            Yc[tree.parent[i]] = Yc[tree.parent[i]] + X @ Yc[i] @ X.T
    return M


# ---------------------------------------------------------------- kinematic terms (control.py:287-345)
def log3(ar, R):
    """pin.log3 away from theta = pi (the controller's orientation errors are small)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    sk = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype=ar.dtype)
    half = ar.num(0.5)
    c = (tr - ar.num(1.0)) * half
    one = ar.num(1.0)
    c = one if c > one else (-one if c < -one else c)
    theta = ar.acos(c)
    n = ar.sqrt(sk @ sk) * half  # sin(theta)
    if theta < ar.num(1e-12):
        return sk * half
    return sk * (theta / (n * 2))


def frame_terms(tree, q, v):
    """Per hand: placement (R, p), LOCAL_WORLD_ALIGNED velocity [6], J [6,nq]
    and dJ v [6] by the world point-velocity form
      J_k = [a_k x (p - o_k); a_k],  dJ_k = [a'_k x (p - o_k) + a_k x (p' - o'_k); a'_k],  a'_k = w_parent x a_k."""
    ar, nq = tree.ar, tree.nq
    q, v = arr(ar, q), arr(ar, v)
    li = tree.liMi(q)
    Rw, ow, ww, od, ax, axd = [], [], [], [], [], []
    for i in range(nq):
        p = tree.parent[i]
        Rp, op, wp, odp = (Rw[p], ow[p], ww[p], od[p]) if p >= 0 else (eye(ar, 3), zeros(ar, 3), zeros(ar, 3), zeros(ar, 3))
        d = Rp @ li[i][1]
        Rw.append(Rp @ li[i][0])
        ow.append(op + d)
        od.append(odp + cross(wp, d))
        a = Rw[i][:, tree.axis[i]].copy()
        ax.append(a)
        axd.append(cross(wp, a))
        ww.append(wp + a * v[i])
    out = []
    for h in range(2):
        j = tree.hand_joint[h]
        d = Rw[j] @ tree.hand[h][1]
        p, pd = ow[j] + d, od[j] + cross(ww[j], d)
        R = Rw[j] @ tree.hand[h][0]
        J = zeros(ar, 6, nq)
        dJv = zeros(ar, 6)
        k = j
        while k >= 0:
            r, rd = p - ow[k], pd - od[k]
            J[:3, k], J[3:, k] = cross(ax[k], r), ax[k]
            dJv = dJv + np.concatenate([cross(axd[k], r) + cross(ax[k], rd), axd[k]]) * v[k]
            k = tree.parent[k]
        out.append(((R, p), np.concatenate([pd, ww[j]]), J, dJv))
    return out


def task_space_terms(tree, q, v, q_des, v_des):
    """control.py:287-345, :368-371 -> J_total [12,nq], J_dot_v_total [12], e [12], e_dot [12]."""
    ar = tree.ar
    cur, des = frame_terms(tree, q, v), frame_terms(tree, q_des, v_des)
    J, dJv, e, ed = [], [], [], []
    for h in range(2):
        (R, p), vel, Jh, dJvh = cur[h]
        (Rd, pd), veld, _, _ = des[h]
        J.append(Jh)
        dJv.append(dJvh)
        e.append(np.concatenate([pd - p, log3(ar, Rd @ R.T)]))  # :326-327
        ed.append(veld - vel)  # :330-331
    return np.vstack(J), np.concatenate(dJv), np.concatenate(e), np.concatenate(ed)


# ---------------------------------------------------------------- control.py:242-410
def default_gains():
    Kp, Kf = 7000.0, 30.0
    fc_bias = np.zeros(12)
    fc_bias[1] = -200.0  # :375
    return dict(Kp=Kp, Kv=2 * math.sqrt(Kp), Kf=Kf, Kt=2 * math.sqrt(Kf), lambda_reg=1e-6, qp_reg=1e-6,
                fc_bias=fc_bias, zero_tau=(1, 2))


def controllaw_terms(tree, q, v, q_des, v_des, terms=None, **gains):
    """The reference's controllaw from :284 to :406 -> dict(M, nle, tau, qdd, xdd, Lambda [2,6,6], fc [12]).
    `terms`: (J_total, J_dot_v_total, e, e_dot) from another source (oracle.control_oracle)."""
    ar = tree.ar
    g = default_gains()
    g.update(gains)
    Kp, Kv, Kf, Kt = (ar.num(g[k]) for k in ("Kp", "Kv", "Kf", "Kt"))
    M = crba(tree, q)  # :284-285
    b = nle(tree, q, v)  # :286
    J_total, J_dot_v_total, e, e_dot = terms if terms is not None else task_space_terms(tree, q, v, q_des, v_des)
    J_total, J_dot_v_total, e, e_dot = (arr(ar, x) if np.asarray(x).dtype != ar.dtype else x
                                        for x in (J_total, J_dot_v_total, e, e_dot))
    Minv = ar.inv(M)
    xdd, fcs, Lams = [], [], []
    for h in range(2):
        J = J_total[6 * h:6 * h + 6]
        eh, edh = e[6 * h:6 * h + 6], e_dot[6 * h:6 * h + 6]
        x_ddot_desired = Kp * eh + Kv * edh  # :338
        Lambda_inv = J @ Minv @ J.T  # :348
        Lambda = ar.inv(Lambda_inv + ar.num(g["lambda_reg"]) * eye(ar, 6))  # :349
        f_c = np.concatenate([Kf * eh[:3], Kt * eh[3:]])  # :352-354
        xdd.append(x_ddot_desired + Lambda @ f_c)  # :357-360
        fcs.append(f_c)
        Lams.append(Lambda)
    x_ddot_des_total = np.concatenate(xdd)
    f_c_total = np.concatenate(fcs)
    f_c_biased = f_c_total + arr(ar, g["fc_bias"])  # :375
    H_qp = J_total.T @ J_total + ar.num(g["qp_reg"]) * eye(ar, tree.nq)  # :381, :386-387
    d_qp = -(J_total.T @ (J_dot_v_total - x_ddot_des_total))  # :382-383
    # quadprog.solve_qp(H, d) minimises 1/2 x^T H x - d^T x without constraints: x = H^-1 d (:395)
    q_ddot_desired = ar.solve(H_qp, d_qp)
    tau = M @ q_ddot_desired + b + J_total.T @ f_c_biased  # :401
    for j in g["zero_tau"]:  # :404-406
        tau[j] = ar.num(0.0)
    return dict(M=M, nle=b, tau=tau, qdd=q_ddot_desired, xdd=x_ddot_des_total, Lambda=np.stack(Lams),
                fc=f_c_total, H=H_qp, d=d_qp)


# ---------------------------------------------------------------- test inputs
def seeded_inertias(nq, seed):
    """Physically valid random body inertias (BodyInertias): each body a box of
    random size and mass, rotated and offset at random in its joint frame."""
    from ikgrasp.model import BodyInertias
    rng = np.random.default_rng(seed)
    mass = rng.uniform(0.2, 3.0, nq)
    com = rng.uniform(-0.08, 0.08, (nq, 3))
    inertia = np.zeros((nq, 6))
    for j in range(nq):
        a = rng.uniform(0.03, 0.25, 3)
        D = mass[j] / 12.0 * np.array([a[1] ** 2 + a[2] ** 2, a[0] ** 2 + a[2] ** 2, a[0] ** 2 + a[1] ** 2])
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        I = Q @ np.diag(D) @ Q.T
        I = 0.5 * (I + I.T)
        inertia[j] = [I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]
    return BodyInertias(mass, com, inertia).validate()


def hanging_passive_model(model, chain=None, below=None):
    """`model` with a serial chain of passive joints (`chain`, head first;
    default: the first passive joint alone) re-parented with its head below
    joint `below` (default: the second joint of arm 0) and moved to the end of
    the q order (parents precede children): a passive chain hanging below an
    arm joint.  Returns (DualArmModel, perm) with new joint k = old joint perm[k]."""
    import copy
    chain = [int(model.passive_q[0])] if chain is None else [int(j) for j in chain]
    below = int(model.arm_q[0][1]) if below is None else int(below)
    passive = set(model.passive_q)
    if not chain or len(set(chain)) != len(chain) or any(j not in passive for j in chain) or below in chain:
        raise ValueError("the chain must be distinct passive joints, and hang below a joint outside it")
    for a, b in zip(chain[:-1], chain[1:]):
        if model.parents[b] != a:
            raise ValueError("the chain must be serial, head first")
    perm = [j for j in range(model.nq) if j not in chain] + chain
    new_of = {old: k for k, old in enumerate(perm)}
    m = copy.deepcopy(model)
    parents = list(model.parents)
    parents[chain[0]] = below
    for old in range(model.nq):
        if old not in chain and parents[old] in chain:
            raise ValueError("the passive chain must end in a leaf")
    m.joint_names = [model.joint_names[o] for o in perm]
    m.parents = [new_of[parents[o]] if parents[o] >= 0 else -1 for o in perm]
    for name in ("R", "t", "axis", "lower", "upper"):
        setattr(m, name, getattr(model, name)[perm].copy())
    if model.Q is not None:
        m.Q = model.Q[perm].copy()
    m.root_q = new_of[int(model.root_q)]
    m.arm_q = np.array([[new_of[int(x)] for x in row] for row in model.arm_q], dtype=np.int32)
    return m.validate(), perm
