"""CPU ORACLE — test infrastructure only, never the product path.

Generic-chain restatement of the grasp-pose IK (`/root/reference/
inverse_geometry.py:41-100`) for the model-generality row:
any URDF tree of revolute + fixed joints, any joint axis direction (Pinocchio's
RX/RY/RZ for +X/+Y/+Z and RevoluteUnaligned, rotation exp(q [e]x) about the
normalised axis, otherwise).  It reads the URDF itself and works in the raw
joint frames with Rodrigues rotations, so it is independent of the product's
model compiler (`ikgrasp/model.py`), which instead re-expresses
non-canonical axes onto X/Y/Z.

Same loop as `ik_oracle.computeqgrasppose`: FK, log6 errors of the two hands
against the cube's hooks, LOCAL frame Jacobians, `np.linalg.pinv(J) @ e`,
q + dt vq, clip to the limits (the collision term is not modelled here).

Parity status: pinned through the Nextage KATs — on the reference's own URDF
this restatement reproduces KAT-1/KAT-2 (`trajectory.json:3-19`, `:258-274`)
in 740 / 736 iterations (`tests/test_generic_model.py`, when the reference
tree is present; the check also runs in `tests/golden/make_golden.py
generic`).  For other robots (the synthetic tilted-axis robot in
`tests/golden/`) no reference outputs exist: the oracle is the statement of
Pinocchio's semantics above.
"""
from __future__ import annotations

import math
import os
import xml.etree.ElementTree as ET

import numpy as np

from oracle import ik_oracle as ik


def _floats(s, n, default):
    if s is None:
        return np.array(default, dtype=np.float64)
    v = [float(t) for t in s.split()]
    assert len(v) == n, s
    return np.array(v)


def _origin(el):
    o = el.find("origin")
    xyz = _floats(o.get("xyz") if o is not None else None, 3, (0.0, 0.0, 0.0))
    rpy = _floats(o.get("rpy") if o is not None else None, 3, (0.0, 0.0, 0.0))
    return ik.urdf_rpy_to_matrix(*rpy), xyz


def rodrigues(e, q):
    """exp(q [e]x) for a unit axis e (JointModelRevoluteUnaligned::calc)."""
    s, c = math.sin(q), math.cos(q)
    K = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
    return np.eye(3) + s * K + (1.0 - c) * (K @ K)


class ChainModel:
    """Joints in Pinocchio order (depth first, siblings by joint name), fixed
    joints folded into frames and into the next joint's placement."""

    def __init__(self, urdf, base_placement=None):
        root = ET.parse(urdf).getroot() if os.path.exists(urdf) else ET.fromstring(urdf)
        links = {l.get("name") for l in root.findall("link")}
        kids, child_links = {}, set()
        for j in root.findall("joint"):
            kids.setdefault(j.find("parent").get("link"), []).append(j)
            child_links.add(j.find("child").get("link"))
        (root_link,) = sorted(links - child_links)
        self.names, self.parent, self.placement, self.axis, self.lower, self.upper = [], [], [], [], [], []
        self.frames = {root_link: (-1, (np.eye(3), np.zeros(3)))}
        self.link_frame = {root_link: (-1, (np.eye(3), np.zeros(3)))}
        self.urdf_root = root

        def visit(link, pj, M):
            for j in sorted(kids.get(link, []), key=lambda e: e.get("name")):
                child = j.find("child").get("link")
                O = ik.se3_mul(M, _origin(j))
                if j.get("type") == "fixed":
                    self.frames[j.get("name")] = (pj, O)
                    self.link_frame[child] = (pj, O)
                    visit(child, pj, O)
                elif j.get("type") == "revolute":
                    if pj < 0 and base_placement is not None:
                        O = ik.se3_mul(base_placement, O)
                    a = _floats(j.find("axis").get("xyz") if j.find("axis") is not None else None, 3, (1, 0, 0))
                    lim = j.find("limit")
                    self.names.append(j.get("name"))
                    self.parent.append(pj)
                    self.placement.append(O)
                    self.axis.append(a / np.linalg.norm(a))
                    self.lower.append(float(lim.get("lower", "0")) if lim is not None else 0.0)
                    self.upper.append(float(lim.get("upper", "0")) if lim is not None else 0.0)
                    idx = len(self.names) - 1
                    I0 = (np.eye(3), np.zeros(3))
                    self.frames[j.get("name")] = (idx, I0)
                    self.link_frame[child] = (idx, I0)
                    visit(child, idx, I0)
                else:
                    raise ValueError(f"joint type {j.get('type')} not modelled")

        visit(root_link, -1, (np.eye(3), np.zeros(3)))
        self.nq = len(self.names)
        self.lower = np.array(self.lower)
        self.upper = np.array(self.upper)

    def fk(self, q):
        oMi = []
        for j in range(self.nq):
            R0, t0 = self.placement[j]
            liMi = (R0 @ rodrigues(self.axis[j], q[j]), t0.copy())
            oMi.append(liMi if self.parent[j] < 0 else ik.se3_mul(oMi[self.parent[j]], liMi))
        return oMi

    def frame(self, oMi, name):
        j, M = self.frames[name]
        return M if j < 0 else ik.se3_mul(oMi[j], M)

    def frame_jacobian_local(self, q, name, oMi=None):
        """computeFrameJacobian (LOCAL): column i over the support = [R_f^T (a_i x (p_f - o_i)); R_f^T a_i]."""
        oMi = oMi if oMi is not None else self.fk(q)
        Rf, pf = self.frame(oMi, name)
        J = np.zeros((6, self.nq))
        i = self.frames[name][0]
        while i >= 0:
            Ri, oi = oMi[i]
            a = Ri @ self.axis[i]
            J[:3, i] = Rf.T @ np.cross(a, pf - oi)
            J[3:, i] = Rf.T @ a
            i = self.parent[i]
        return J

    def geometry_placements(self, oMi):
        """World placement of every <collision> of every link (link order of the URDF)."""
        out = {}
        for link in self.urdf_root.findall("link"):
            j, M = self.link_frame[link.get("name")]
            for k, c in enumerate(link.findall("collision")):
                G = ik.se3_mul(M, _origin(c))
                out[f"{link.get('name')}_{k}"] = G if j < 0 else ik.se3_mul(oMi[j], G)
        return out


def cube_hooks(cube_urdf, hooks=("LARM_HOOK", "RARM_HOOK")):
    c = ChainModel(cube_urdf)
    return [c.frames[h][1] for h in hooks]


def damped_step(lam):
    """J^T (J J^T + lam I)^-1 e: ik_oracle.computeqgrasppose's `lam > 0` step."""
    return lambda J, e: J.T @ np.linalg.solve(J @ J.T + lam * np.eye(len(e)), e)


def lstsq_step(J, e):
    """The minimum-norm least-squares step by LAPACK's gelsd instead of pinv's SVD product."""
    return np.linalg.lstsq(J, e, rcond=None)[0]


def computeqgrasppose(model, hooks, q0, cube_R, cube_t, hands=("LARM_EFF", "RARM_EFF"), max_iters=ik.MAX_ITERS,
                      dt=ik.DT, eps=ik.EPSILON, step=None):
    """inverse_geometry.py:41-100 on a generic model (no collision term).
    `step(J, e)` replaces np.linalg.pinv(J) @ e (np.linalg.lstsq for the
    rounding check of the family fixtures; `damped_step(lam)`).
    Returns (q, converged, updates, (|eL|, |eR|))."""
    cube = (np.asarray(cube_R, dtype=np.float64), np.asarray(cube_t, dtype=np.float64))
    targets = [ik.se3_mul(cube, hk) for hk in hooks]
    q = np.array(q0, dtype=np.float64).copy()

    def errors(q):
        oMi = model.fk(q)
        es = [ik.log6(ik.se3_mul(ik.se3_inv(model.frame(oMi, h)), T)) for h, T in zip(hands, targets)]
        return oMi, es

    for it in range(max_iters):
        oMi, (eL, eR) = errors(q)
        nL, nR = np.linalg.norm(eL), np.linalg.norm(eR)
        if nL < eps and nR < eps:
            return q, True, it, (nL, nR)
        J = np.vstack([model.frame_jacobian_local(q, h, oMi) for h in hands])
        e = np.hstack([eL, eR])
        vq = step(J, e) if step is not None else np.linalg.pinv(J) @ e
        q = np.minimum(np.maximum(model.lower, q + vq * dt), model.upper)
    _, (eL, eR) = errors(q)
    return q, False, max_iters, (np.linalg.norm(eL), np.linalg.norm(eR))


def computeqgrasppose_mp(model, hooks, q0, cube_R, cube_t, hands=("LARM_EFF", "RARM_EFF"), max_iters=ik.MAX_ITERS,
                         dt=ik.DT, eps=ik.EPSILON, dps=32):
    """The loop of `computeqgrasppose` in `dps`-digit arithmetic (mpmath) from
    the float64 model constants and inputs, rounded to float64 at the end: what
    the float64 loop approximates (ik_oracle.computeqgrasppose_mp for a generic
    model; the step is J^T (J J^T)^-1 e, pinv(J) e for a J of full row rank).
    Returns (q, converged, updates, (|eL|, |eR|))."""
    import mpmath as mp
    mp.mp.dps = dps
    f = mp.mpf
    mat = lambda A: [[f(float(A[i][j])) for j in range(3)] for i in range(3)]
    vec = lambda v: [f(float(x)) for x in v]
    mm = lambda A, B: [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]
    mv = lambda A, v: [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]
    mtv = lambda A, v: [A[0][i] * v[0] + A[1][i] * v[1] + A[2][i] * v[2] for i in range(3)]
    tr = lambda A: [[A[j][i] for j in range(3)] for i in range(3)]
    se3 = lambda A, B: (mm(A[0], B[0]), [A[1][i] + mv(A[0], B[1])[i] for i in range(3)])
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def rod(e, q):  # exp(q [e]x)
        s, c = mp.sin(q), 1 - mp.cos(q)
        K = [[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]]
        KK = mm(K, K)
        return [[(1 if i == j else 0) + s * K[i][j] + c * KK[i][j] for j in range(3)] for i in range(3)]

    n = model.nq
    P = [(mat(R0), vec(t0)) for R0, t0 in model.placement]
    axes = [vec(a) for a in model.axis]
    frames = [(model.frames[h][0], (mat(model.frames[h][1][0]), vec(model.frames[h][1][1]))) for h in hands]
    cube = (mat(cube_R), vec(cube_t))
    tgts = [se3(cube, (mat(hk[0]), vec(hk[1]))) for hk in hooks]
    lo, hi = vec(model.lower), vec(model.upper)
    q = vec(q0)
    for it in range(max_iters + 1):
        oMi = []
        for j in range(n):
            l = (mm(P[j][0], rod(axes[j], q[j])), P[j][1])
            oMi.append(l if model.parent[j] < 0 else se3(oMi[model.parent[j]], l))
        es, rows = [], []
        for (j, M), (TR, Tt) in zip(frames, tgts):
            Rh, th = se3(oMi[j], M)
            es.append(ik.log6_mp(mm(tr(Rh), TR), mtv(Rh, [Tt[i] - th[i] for i in range(3)])))
            J = [[f(0)] * n for _ in range(6)]
            i = j
            while i >= 0:  # LOCAL: column = [R_f^T (a x (p_f - o_i)); R_f^T a]
                a = mv(oMi[i][0], axes[i])
                lin, ang = mtv(Rh, cross(a, [th[r] - oMi[i][1][r] for r in range(3)])), mtv(Rh, a)
                for r in range(3):
                    J[r][i], J[3 + r][i] = lin[r], ang[r]
                i = model.parent[i]
            rows += J
        nL, nR = (mp.sqrt(sum(x * x for x in e)) for e in es)
        if it >= max_iters or (nL < eps and nR < eps):
            break
        Jm = mp.matrix(rows)
        x = Jm.T * mp.lu_solve(Jm * Jm.T, mp.matrix(es[0] + es[1]))
        q = [min(max(lo[k], q[k] + x[k] * f(dt)), hi[k]) for k in range(n)]
    conv = bool(nL < eps and nR < eps) and it < max_iters
    return np.array([float(v) for v in q]), conv, it, (float(nL), float(nR))
