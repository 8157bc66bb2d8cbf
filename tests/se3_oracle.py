"""CPU ORACLE -- test infrastructure only, never the product path.

The SE(3) logarithm and exponential (pin.log6 / pin.exp6, [v; w]) three times:

  log6_mp / exp6_mp / interpolate_mp   50-digit mpmath, evaluated FROM THE FLOAT
            INPUTS exactly as given (a rounded R is taken as it stands), with no
            branches: theta = atan2(|skew|/2, (tr - 1)/2), w = theta skew / (2 |skew|/2),
            alpha = theta sin / (2 (1 - cos)), beta = 1/theta^2 - sin / (2 theta (1 - cos)).
  log6_ref  the reference restated in numpy: float64 is Pinocchio's log6 with its
            own branches (oracle/ik_oracle.py); float32 evaluates the closed forms in
            np.float32 with the atan2 angle, guarded only at theta = 0 (Pinocchio
            has no fp32 form and an acos angle is meaningless near 0 in fp32: the
            project's one documented deviation).
  log6_accurate  a float64 evaluation that tests/test_se3.py proves to be within
            8 eps max(1, |p|) of log6_mp on every fixture row; the GPU tests use it for
            inputs that only exist at run time (FK outputs), where mpmath may be absent.

Near pi (theta >= pi - 1e-2) every one of them takes the axis from the diagonal,
w_i = sign(skew_i) theta sqrt((R_ii - c) / (1 - c)) with c = (tr - 1)/2 and Pinocchio's
sign rule (skew_i > 0 -> +, else -), which is the definition the kernels implement.
skew / |skew| of a ROUNDED rotation is ill-conditioned there: |skew| = 2 sin(theta) -> 0
while each entry keeps a rounding error of eps, so the direction it gives is off by
eps / sin(theta) (1e-7 at pi - 1e-9) and no amount of precision in the evaluation
brings it back -- the information is in the diagonal.  With c taken from the trace
itself the radicand is the plain sum (R_ii - R_jj - R_kk + 1)/2, which float64 can
form exactly (math.fsum): where an axis component is zero that sum is a rounding
residue of the matrix (1e-16, its root 1e-8), the same number in every precision.

mpmath is imported by the functions that need it, so that the GPU tests can import
gates() and log6_accurate() without it.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

DPS = 50
NEAR_PI = math.pi - 1e-2
PREC3 = {"f64": 2.0 ** -13, "f32": float(np.float32(0.1))}  # Prec<T>::kPrec3 (csrc/ikg_device.hpp)
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
AXIS_CLASSES = ("coordinate", "zero-component", "random")


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ---------------------------------------------------------------- 50 digits
def _log6_mpf(R, p):
    """R 3x3, p 3x1 mp matrices -> (v, w, theta) in mp"""
    mp = _mp()
    skew = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    st = mp.sqrt(sum(x * x for x in skew)) / 2
    ct = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    theta = mp.atan2(st, ct)
    if theta == 0:
        return p, mp.matrix([0, 0, 0]), theta
    if theta >= NEAR_PI:
        w = mp.matrix([0, 0, 0])
        for i in range(3):
            t = (R[i, i] - ct) / (1 - ct)
            w[i] = (1 if skew[i] > 0 else -1) * (theta * mp.sqrt(t) if t > 0 else 0)
    else:
        w = skew * (theta / (2 * st))
    s, c = mp.sin(theta), mp.cos(theta)
    al = theta * s / (2 * (1 - c))
    be = 1 / theta ** 2 - s / (2 * theta * (1 - c))
    wxp = mp.matrix([w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]])
    v = al * p - wxp / 2 + (be * (w.T * p)[0]) * w
    return v, w, theta


def _exp6_mpf(v, w):
    """v, w 3x1 mp matrices -> (R, t) in mp"""
    mp = _mp()
    t = mp.sqrt(sum(x * x for x in w))
    W = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if t == 0:
        return mp.eye(3), v
    a, b, c = mp.sin(t) / t, (1 - mp.cos(t)) / t ** 2, (t - mp.sin(t)) / t ** 3
    return mp.eye(3) + a * W + b * (W * W), (mp.eye(3) + b * W + c * (W * W)) * v


def _split(M):
    mp = _mp()
    M = [float(x) for x in np.asarray(M).reshape(12)]  # float32 values convert exactly
    return mp.matrix([M[0:3], M[3:6], M[6:9]]), mp.matrix(M[9:12])


def _flat(R, t):
    return np.array([float(R[i, j]) for i in range(3) for j in range(3)] + [float(t[i]) for i in range(3)])


def log6_mp(M):
    """M [12] (R row-major, then p; any float type) -> [6] float64 = [v; w], the
    50-digit value rounded once"""
    v, w, _ = _log6_mpf(*_split(M))
    return np.array([float(x) for x in v] + [float(x) for x in w])


def exp6_mp(xi):
    """xi [6] = [v; w] -> [12], the 50-digit value rounded once"""
    mp = _mp()
    xi = [float(x) for x in np.asarray(xi).reshape(6)]
    return _flat(*_exp6_mpf(mp.matrix(xi[:3]), mp.matrix(xi[3:])))


def interpolate_mp(A, B, alpha):
    """pin.SE3.Interpolate(A, B, alpha) = A exp6(alpha log6(A^-1 B)) in 50 digits; A, B
    (R [3,3], t [3]) float arrays -> [12]"""
    mp = _mp()
    Ra, ta = mp.matrix(np.asarray(A[0], dtype=np.float64).tolist()), mp.matrix(np.asarray(A[1], dtype=np.float64).tolist())
    Rb, tb = mp.matrix(np.asarray(B[0], dtype=np.float64).tolist()), mp.matrix(np.asarray(B[1], dtype=np.float64).tolist())
    v, w, _ = _log6_mpf(Ra.T * Rb, Ra.T * (tb - ta))
    al = mp.mpf(float(alpha))
    Re, te = _exp6_mpf(al * v, al * w)
    return _flat(Ra * Re, ta + Ra * te)


def rotation_mp(axis, theta):
    """Rodrigues in 50 digits: axis [3] floats (normalised here), theta a float, an
    mp number or the string "pi" (sin = 0, cos = -1 exactly: R = 2 a a^T - 1 is
    symmetric, its skew part exactly zero) -> mp 3x3"""
    mp = _mp()
    a = mp.matrix([float(x) for x in axis])
    a = a / mp.sqrt(sum(x * x for x in a))
    if isinstance(theta, str):
        assert theta == "pi"
        s, c = mp.mpf(0), mp.mpf(-1)
    else:
        s, c = mp.sin(theta), mp.cos(theta)
    K = mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return c * mp.eye(3) + s * K + (1 - c) * (a * a.T)


# ---------------------------------------------------------------- the reference restated
def _log6_ref32(M):
    f = np.float32
    M = np.asarray(M, dtype=f).reshape(12)
    R, p = M[:9].reshape(3, 3), M[9:]
    skew = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype=f)
    st = f(0.5) * np.sqrt(skew[0] * skew[0] + skew[1] * skew[1] + skew[2] * skew[2])
    ct = f(0.5) * (R[0, 0] + R[1, 1] + R[2, 2] - f(1))
    theta = np.arctan2(st, ct)
    if theta == 0:
        return np.concatenate([p, np.zeros(3, f)])
    s, c = np.sin(theta), np.cos(theta)
    if theta >= f(math.pi) - f(1e-2):  # Pinocchio's near-pi axis
        cphi = np.cos(theta - f(math.pi))
        beta = theta * theta / (f(1) + cphi)
        tmp = (np.diag(R) + cphi) * beta
        w = np.where(skew > 0, f(1), f(-1)) * np.sqrt(np.maximum(tmp, f(0)))
    else:
        w = (f(0.5) * (theta / s)) * skew
    # the closed forms, with 1 - cos = 2 sin^2(theta/2): in fp32 cos(theta) rounds to 1 below 2e-4
    h = f(0.5) * theta
    alpha = h * np.cos(h) / np.sin(h)
    beta = (f(1) - alpha) / (theta * theta)
    v = alpha * p - f(0.5) * np.cross(w, p).astype(f) + (beta * np.dot(w, p)) * w
    return np.concatenate([v, w]).astype(f)


def log6_ref(M, dtype="f64"):
    """M [12] -> [6] in `dtype`'s arithmetic (see the module docstring)"""
    if dtype == "f32":
        return _log6_ref32(M)
    from oracle import ik_oracle
    M = np.asarray(M, dtype=np.float64).reshape(12)
    return ik_oracle.log6((M[:9].reshape(3, 3), M[9:]))


# ---------------------------------------------------------------- accurate float64
def log6_accurate(M):
    """M [N,12] or [12] float64 -> [N,6] / [6]: atan2 angle, theta / sin(theta) (the sine
    being |skew|/2), the near-pi axis from the diagonal with an exactly summed radicand"""
    M = np.asarray(M, dtype=np.float64)
    one = M.ndim == 1
    M = M.reshape(-1, 12)
    R, p = M[:, :9].reshape(-1, 3, 3), M[:, 9:]
    skew = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    st = 0.5 * np.sqrt(np.sum(skew * skew, axis=1))
    ct = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0)
    theta = np.arctan2(st, ct)
    t2 = theta * theta
    small = theta < 1e-2
    with np.errstate(divide="ignore", invalid="ignore"):
        # theta / sin(theta) with the sine the angle was formed from: |skew|/2 = rho sin(theta), rho = 1 + O(eps)
        # for a rounded rotation, and unlike sin(theta) it keeps its relative accuracy up to pi
        f = np.where(theta > 0, theta / np.where(st > 0, st, 1.0), 1.0)
        h = 0.5 * theta
        alpha = np.where(small, 1.0 - t2 / 12.0 - t2 * t2 / 720.0 - t2 * t2 * t2 / 30240.0, h * np.cos(h) / np.sin(h))
        beta = np.where(small, 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0 + t2 * t2 * t2 / 1209600.0,
                        (1.0 - alpha) / np.where(t2 > 0, t2, 1.0))
    w = (0.5 * f)[:, None] * skew
    for i in np.nonzero(theta >= NEAR_PI)[0]:
        d = [R[i, 0, 0], R[i, 1, 1], R[i, 2, 2]]
        den = math.fsum([3.0, -d[0], -d[1], -d[2]])  # 2 (1 - c)
        for k in range(3):
            num = math.fsum([d[k], -d[(k + 1) % 3], -d[(k + 2) % 3], 1.0])  # 2 (R_kk - c)
            w[i, k] = (1.0 if skew[i, k] > 0 else -1.0) * (theta[i] * math.sqrt(num / den) if num > 0 else 0.0)
    wp = np.sum(w * p, axis=1)
    v = alpha[:, None] * p - 0.5 * np.cross(w, p) + (beta * wp)[:, None] * w
    out = np.concatenate([v, w], axis=1)
    return out[0] if one else out


# ---------------------------------------------------------------- the fixture and its gates
def load():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se3_cases.npz"))


def mid_band(theta, dtype="f64"):
    """where log6<double> and log6_iter<double> form theta / (|skew|/2) with the acos angle.
    theta = kPrec3 itself counts: acos carries eps / theta = 1e-12 there, so the rounding
    decides on which side of the Taylor edge such a row is evaluated."""
    return (theta >= PREC3[dtype]) & (theta < NEAR_PI)


def gates(d, dtype, envelope=None):
    """Per row of the log fixture `d` (load()) of `dtype`: (rows, gate [n,6]).
    gate = max(16 ref_err[bucket], floor), floor = 4 eps_T max(1, |p|) on v and
    4 eps_T max(1, theta) on w.  envelope (log6<double>, log6_iter<double> between
    kPrec3 and pi - 1e-2): + envelope_gate() of that kind."""
    rows = np.nonzero(d["dtype"] == (0 if dtype == "f64" else 1))[0]
    eps = EPS[dtype]
    pn = np.linalg.norm(d["M"][rows, 9:], axis=1)
    th = d["theta"][rows]
    re = d["ref_err"][d["bucket"][rows]]  # [n, 2] = (w, v)
    g = np.empty((len(rows), 6))
    g[:, :3] = np.maximum(16 * re[:, 1], 4 * eps * np.maximum(1.0, pn))[:, None]
    g[:, 3:] = np.maximum(16 * re[:, 0], 4 * eps * np.maximum(1.0, th))[:, None]
    if envelope:
        assert dtype == "f64"
        g += envelope_gate(d, th, pn, envelope)
    return rows, g


def envelope_gate(d, theta, pn, kind="stated"):
    """The default form's envelope inside the mid band (0 outside), [..., 6].  env = eps / sin(theta):
    acos((tr - 1)/2) is off by that much and theta / (|skew|/2) does not cancel it.  Each K is the
    worst err / envelope of the form restated in numpy on the fixture's rows (make_se3_golden.py).
    w: 4 K_meas env (K_meas = 1.00);
    v, kind "stated": 4 K_meas_v env |p|, w's envelope times |p|.  K_meas_v =
       4.55e3, not O(1): alpha = f/2 (1 + cos) carries f's RELATIVE error eps / sin^2(theta) and
       v = alpha p + ..., so env |p| is short by 1 / sin(theta) and K makes up for it at the
       smallest angle (1.3e-4 rad) -- and is 1 / sin(theta) too generous everywhere above it;
    v, kind "derived": 4 Kv_meas env |p| / sin(theta) (Kv_meas = 0.98), which follows the error
       over the whole band and is never above the stated one: what the other tests use."""
    theta, pn = np.asarray(theta, dtype=np.float64), np.asarray(pn, dtype=np.float64)
    mid = mid_band(theta)
    s = np.sin(np.where(mid, theta, 1.0))
    env = np.where(mid, EPS["f64"] / s, 0.0)
    g = np.empty(theta.shape + (6,))
    g[..., 3:] = (4 * float(d["K_meas"]) * env)[..., None]
    if kind == "stated":
        g[..., :3] = (4 * float(d["K_meas_v"]) * env * pn)[..., None]
    else:
        assert kind == "derived"
        g[..., :3] = (4 * float(d["Kv_meas"]) * env / s * pn)[..., None]
    return g
