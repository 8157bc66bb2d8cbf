"""Problems for the rare branch of the fp64 pair loop's SE(3) log (log6_iter<COLD>: the
small-angle forms and the near-pi axis behind one wave-uniform branch), chosen on the CPU with
the C oracle.  At the default parameters a hand's rotation error falls below kPrec3 = 1.22e-4
only 200 updates after its problem has passed at eps = 1e-3; with eps = 1e-6 and dt = 0.05 a
problem that passes has crossed kPrec3 first (|w| <= |e| < 1e-6), and one that never passes
and ends with both angles far above kPrec3 has not."""
import numpy as np

from oracle import c_oracle, ik_oracle

PARAMS = dict(eps=1e-6, dt=0.05, max_iters=1000)
KPREC3 = 1.220703125e-04


def roll(tg, a):
    """The targets' rotations times Rx(a): no longer a rotation about z (the general loop)."""
    out = np.array(tg, dtype=np.float64).reshape(-1, 12).copy()
    c, s = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    out[:, :9] = (out[:, :9].reshape(-1, 3, 3) @ rx).reshape(-1, 9)
    return out


def oracle(tg, q0, **kw):
    p = dict(PARAMS, **kw)
    return c_oracle.solve_ex(tg, q0, c_oracle.QR_STEP, **p)


def end_angles(tg, q):
    """Rotation angle of either hand's error at q (numpy oracle FK and log)."""
    out = np.empty((len(tg), 2))
    for i, (t, qi) in enumerate(zip(np.asarray(tg).reshape(-1, 12), q)):
        L, R = ik_oracle.hook_targets(t[:9].reshape(3, 3), t[9:])
        eL, eR = ik_oracle.hand_errors(qi, L, R)
        out[i] = np.linalg.norm(eL[3:]), np.linalg.norm(eR[3:])
    return out


def pick(pool, q0, n_cross, n_never):
    """Rows of pool: n_cross that pass after crossing kPrec3, n_never whose angles end > 10 kPrec3
    without passing; with their oracle solutions under PARAMS."""
    q, c, it, err = oracle(pool, q0)
    ang = end_angles(pool, q)
    cross = np.nonzero(c)[0]
    never = np.nonzero(~c & (ang.min(axis=1) > 10 * KPREC3))[0]
    assert len(cross) >= n_cross and len(never) >= n_never, (len(cross), len(never))
    return cross[:n_cross], never[:n_never]
