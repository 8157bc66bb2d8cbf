"""Fixture of the SE(3) log / exp accuracy tests (tests/test_se3.py,
tests/test_gpu_se3.py) -> tests/golden/se3_cases.npz, answered by
tests/se3_oracle.py in 50 digits.  Seconds of CPU; the file is written with fixed
zip timestamps, so a second run reproduces it bit for bit.

log rows   M [12] = R row-major, then p.  R is built in 50 digits from (axis,
           theta) and rounded once to float64 (dtype 0) or float32 (dtype 1);
           `exact` is log6_mp of that rounded matrix, `ref` is log6_ref of it.
  angles   ANGLES below: 0 (R = 1 bitwise), the Taylor edge kPrec3 (1 -+ 2^-20) of
           both dtypes, the band above it where the acos angle is noisy, pi/2
           (the alpha switch), the near-pi edge pi - 1e-2 -+ 1e-6, and pi itself
           (sin = 0, cos = -1 exactly: coordinate and zero-component axes only, whose
           skew part is exactly zero -- the sign select at a tie)
  axes     +-x, +-y, +-z; six axes with one component exactly zero; 16 random
  p        by row: |p| = 1e-3, |p| = 10, then 0 and |p| ~ 1 in turn
  clamps   the diagonal of 1, and of a rotation by 1e-9, nudged up by 4 ulps (tr > 3) and diag(1, -1, -1)-like
           matrices nudged down (tr < -1); `exact` is the un-nudged matrix's value
  bucket   (angle, axis class, dtype); ref_err[bucket] = (max |ref - exact| on w, on v)
  K_meas   (w; K_meas_v: v, by |p|) the worst err / (eps / sin theta) of the three-line default form
           theta = acos((tr - 1)/2), f = theta / (|skew|/2), w = f/2 skew on the
           float64 rows between kPrec3 and pi - 1e-2, where log6<double> and
           log6_iter<double> evaluate it; Kv_meas: the worst err / (eps |p| / sin^2 theta) of
           its v, alpha = f/2 (1 + cos theta) carrying f's relative error
exp rows   xi = [v; theta axis] -> exp6_mp, planner_oracle.exp6
interp     A random, B = A exp6(xi) in 50 digits rounded to float64, alpha in ALPHAS (every
           angle but pi itself, where the signs of the axis are those of rounding noise; pi with
           A's rotation the identity, a coordinate axis and alpha 0 and 1, where they are not),
           and per alpha rows with |alpha w| = kPrec3 (1 -+ 2^-20), exp6's own Taylor
           edge: interpolate_mp, planner_oracle.se3_interpolate

python tests/golden/make_se3_golden.py
"""
import io
import math
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import se3_oracle as so  # noqa: E402

K64, K32 = so.PREC3["f64"], so.PREC3["f32"]
D = 2.0 ** -20
PI = "pi"
ANGLES = (0.0, 1e-9, 1e-8, 1e-5, K64 * (1 - D), K64, K64 * (1 + D), 1.3e-4, 2e-4, 1e-3, 1e-2, K32 * (1 - D), K32,
          K32 * (1 + D), 1.0, math.pi / 2 * (1 - 1e-6), math.pi / 2 * (1 + 1e-6), 3.0, 3.13, math.pi - 1e-2 - 1e-6,
          math.pi - 1e-2 + 1e-6, math.pi - 1e-3, math.pi - 1e-6, math.pi - 1e-9, PI)
CLAMP_HI, CLAMP_LO = len(ANGLES), len(ANGLES) + 1  # angle ids of the two clamp groups
ALPHAS = (0.0, 0.3, 0.5, 1.0, 1.5)
NPT = (np.float64, np.float32)


def axes(rng):
    """[(class, axis)]: 6 coordinate, 6 zero-component, 16 random"""
    out = [(0, s * np.eye(3)[k]) for k in range(3) for s in (1.0, -1.0)]
    for k in range(3):
        for s in (1.0, -1.0):
            a = rng.normal(size=3)
            a[k] = 0.0
            a[(k + 1) % 3] *= s
            out.append((1, a / np.linalg.norm(a)))
    for _ in range(16):
        a = rng.normal(size=3)
        out.append((2, a / np.linalg.norm(a)))
    return out


def translation(rng, i):
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    return (1e-3 * u, 10.0 * u, np.zeros(3), rng.uniform(0.8, 1.2) * u)[(0, 1, 2, 0, 1, 3)[i % 6]]


def rounded(Rmp, npt):
    return np.array([[float(Rmp[i, j]) for j in range(3)] for i in range(3)]).astype(npt)


def make_log(out):
    rng = np.random.default_rng(20)
    rows = []  # (M, exact, ref, angle id, class, dtype, theta)
    for dt, npt in enumerate(NPT):
        name = ("f64", "f32")[dt]
        for ai, ang in enumerate(ANGLES):
            for k, (cls, ax) in enumerate(axes(rng)):
                if ang == PI and cls == 2:
                    continue
                R = np.eye(3, dtype=npt) if ang == 0.0 else rounded(so.rotation_mp(ax, ang), npt)
                M = np.concatenate([R.reshape(9), translation(rng, k).astype(npt)]).astype(npt)
                rows.append((M.astype(np.float64), so.log6_mp(M), so.log6_ref(M, name).astype(np.float64), ai, cls, dt,
                             math.pi if ang == PI else ang))
        # the clamps: exact = the un-nudged matrix's value
        # 4 ulps away from 0: the trace leaves [-1, 3] in any order of summation (1 ulp of 1 is half an ulp of 3)
        up = lambda x: npt(x) + npt(4 * np.sign(x)) * np.spacing(npt(1))
        for k, nudge in enumerate(((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2))):
            # the last three about a rotation by 1e-9 (its diagonal rounds to 1): a skew part to go wrong with
            R0 = np.eye(3, dtype=npt) if k < 3 else rounded(so.rotation_mp(rng.normal(size=3), 1e-9), npt)
            assert (np.diag(R0) == 1).all()
            R = R0.copy()
            for j in nudge:
                R[j, j] = up(1.0)
            p = translation(rng, k).astype(npt)
            M, M0 = np.concatenate([R.reshape(9), p]).astype(npt), np.concatenate([R0.reshape(9), p]).astype(npt)
            assert M[0] + M[4] + M[8] > 3
            rows.append((M.astype(np.float64), so.log6_mp(M0), so.log6_ref(M, name).astype(np.float64), CLAMP_HI, 0, dt, 0.0))
        for k, (keep, nudge) in enumerate(((0, (1,)), (0, (1, 2)), (1, (0,)), (1, (0, 2)), (2, (0,)), (2, (0, 1)))):
            R0 = -np.eye(3, dtype=npt)
            R0[keep, keep] = 1
            R = R0.copy()
            for j in nudge:
                R[j, j] = up(-1.0)
            p = translation(rng, k).astype(npt)
            M, M0 = np.concatenate([R.reshape(9), p]).astype(npt), np.concatenate([R0.reshape(9), p]).astype(npt)
            assert M[0] + M[4] + M[8] < -1
            rows.append((M.astype(np.float64), so.log6_mp(M0), so.log6_ref(M, name).astype(np.float64), CLAMP_LO, 0, dt,
                         math.pi))
    M, exact, ref = (np.array([r[i] for r in rows]) for i in range(3))
    ai, cls, dt = (np.array([r[i] for r in rows], dtype=np.int32) for i in (3, 4, 5))
    theta = np.array([r[6] for r in rows])
    keys = sorted(set(zip(ai.tolist(), cls.tolist(), dt.tolist())))
    index = {k: i for i, k in enumerate(keys)}
    bucket = np.array([index[k] for k in zip(ai.tolist(), cls.tolist(), dt.tolist())], dtype=np.int32)
    ref_err = np.zeros((len(keys), 2))
    for b in range(len(keys)):
        sel = bucket == b
        assert sel.sum() >= (16 if keys[b][1] == 2 else 6), (keys[b], sel.sum())
        e = np.abs(ref[sel] - exact[sel])
        ref_err[b] = e[:, 3:].max(), e[:, :3].max()
    assert np.isfinite(ref_err).all() and np.isfinite(ref).all()
    bdt = np.array([k[2] for k in keys])
    for d_, lim in ((0, 1e-6), (1, 2e-3)):
        worst = ref_err[bdt == d_].max()
        print(f"log6_ref vs exact, dtype {d_}: worst bucket {worst:.3e} (limit {lim:g})")
        assert worst <= lim, "the reference alone leaves its limit: the input set is wrong"
    # the documented envelope of the default form on the float64 mid-band rows
    mid = (dt == 0) & so.mid_band(theta) & (ai < CLAMP_HI)
    R = M[mid, :9].reshape(-1, 3, 3)
    pn = np.linalg.norm(M[mid, 9:], axis=1)
    skew = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    st = 0.5 * np.sqrt(np.sum(skew * skew, axis=1))
    ct = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0)
    th = np.arccos(ct)
    f = th / st
    w = (0.5 * f)[:, None] * skew
    env = so.EPS["f64"] / np.sin(theta[mid])
    rw = np.abs(w - exact[mid, 3:]).max(axis=1) / env
    # v with the same f: alpha = f/2 (1 + cos) (cos >= 0) or theta sin / (2 (1 - cos)), beta = (1 - alpha) / theta^2
    alpha = np.where(ct >= 0, 0.5 * f * (1 + ct), th * st / (2 * (1 - ct)))
    beta = (1 - alpha) / (th * th)
    p = M[mid, 9:]
    v = alpha[:, None] * p - 0.5 * np.cross(w, p) + (beta * np.sum(w * p, axis=1))[:, None] * w
    # v inherits f's relative error eps / sin^2 through alpha: measured by env |p| / sin(theta)
    rv = np.abs(v - exact[mid, :3]).max(axis=1) / (env / np.sin(theta[mid]) * np.maximum(pn, 1e-300))
    rv[pn == 0] = 0.0
    # the same error on the scale of the stated envelope, env |p|
    rvs = rv / np.sin(theta[mid])
    for a in sorted(set(ai[mid].tolist())):
        s = ai[mid] == a
        print(f"  default form at theta = {ANGLES[a]:.6g}: w err/env {rw[s].max():.3f} (abs "
              f"{(rw[s] * env[s]).max():.2e}), v err/(env |p| / sin) {rv[s].max():.3g} (abs {(rv[s] * env[s] / np.sin(theta[mid][s]) * pn[s]).max():.2e})")
    out.update(M=M, exact=exact, ref=ref, angle_id=ai, axis_class=cls, dtype=dt, theta=theta, bucket=bucket,
               bucket_key=np.array(keys, dtype=np.int32), ref_err=ref_err, K_meas=np.array(rw.max()),
               Kv_meas=np.array(rv.max()), K_meas_v=np.array(rvs.max()))
    print(f"log rows {len(rows)}, buckets {len(keys)}, K_meas {rw.max():.3f} (w), {rvs.max():.4g} (v, by env |p|), "
          f"Kv_meas {rv.max():.3g} (v, by env |p| / sin)")


def _xi(rng, ax, ang, vn):
    mp = so._mp()
    a = mp.matrix([float(x) for x in ax])
    a = a / mp.sqrt(sum(x * x for x in a))
    th = mp.pi if ang == PI else mp.mpf(ang)
    v = rng.normal(size=3)
    v *= vn / np.linalg.norm(v)
    return mp.matrix(v.tolist()), th * a


def make_exp(out):
    from oracle import planner_oracle as po
    rng = np.random.default_rng(21)
    rows = []
    for ai, ang in enumerate(ANGLES):
        ax = axes(rng)
        for cls, a in (ax[1], ax[7], ax[12], ax[13]):
            v, w = _xi(rng, a, ang, 1.0)
            xi = np.array([float(x) for x in v] + [float(x) for x in w])
            R, t = po.exp6(xi)
            rows.append((xi, so.exp6_mp(xi), np.concatenate([R.reshape(9), t]), ai))
    xi, exact, ref = (np.array([r[i] for r in rows]) for i in range(3))
    ai = np.array([r[3] for r in rows], dtype=np.int32)
    err = np.zeros((len(ANGLES), 2))
    for a in range(len(ANGLES)):
        e = np.abs(ref[ai == a] - exact[ai == a])
        err[a] = e[:, :9].max(), e[:, 9:].max()
    assert np.isfinite(err).all() and err.max() <= 1e-6, err.max()
    out.update(exp_xi=xi, exp_exact=exact, exp_ref=ref, exp_angle_id=ai, exp_ref_err=err)
    print(f"exp rows {len(rows)}: planner_oracle.exp6 vs exact, worst {err.max():.3e}")


def make_interp(out):
    from scipy.spatial.transform import Rotation
    from oracle import planner_oracle as po
    rng = np.random.default_rng(22)
    # not pi itself: the skew part of A^T B is then rounding noise, and Pinocchio's near-pi axis takes each
    # component's sign from it -- the log of such a pair is not a function of the placements (at alpha = 1
    # the 50-digit value itself misses B by 1.5); the log rows have pi with an exactly symmetric R
    cases = [(ai, ang, al) for ai, ang in enumerate(ANGLES) for al in ALPHAS if ang != PI]
    # exp6's Taylor edge |alpha w| = kPrec3 (1 -+ 2^-20): angle ids after the clamps'
    edge = [(CLAMP_LO + 1 + k, K64 * (1 + s * D) / al, al) for k, (al, s) in
            enumerate((al, s) for al in ALPHAS[1:] for s in (-1, 1))]
    rows = []
    for ai, ang, al in cases + edge:
        ax = axes(rng)
        for j, (cls, a) in enumerate((ax[8], ax[14]) if ai < CLAMP_HI else (ax[14], ax[15])):
            mp = so._mp()
            Ra = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
            ta = rng.uniform(-0.5, 1.0, 3)
            v, w = _xi(rng, a, ang, 0.3)
            Re, te = so._exp6_mpf(v, w)
            Am = mp.matrix(Ra.tolist())
            B = so._flat(Am * Re, mp.matrix(ta.tolist()) + Am * te)
            Rb, tb = B[:9].reshape(3, 3), B[9:]
            R, t = po.se3_interpolate((Ra, ta), (Rb, tb), al)
            rows.append((np.concatenate([Ra.reshape(9), ta]), B, al, np.concatenate([R.reshape(9), t]),
                         so.interpolate_mp((Ra, ta), (Rb, tb), al), ai, math.pi if ang == PI else ang))
    # pi where it is a function of the placements: A's rotation the identity, B's a half turn about a
    # coordinate axis, so that A^T B is B's own bitwise symmetric matrix in any arithmetic (a tie in every
    # sign select), and alpha 0 and 1, which do not depend on the axis' sign
    for k in range(3):
        for al in (0.0, 1.0):
            ta, tb = rng.uniform(-0.5, 1.0, 3), rng.uniform(-0.5, 1.0, 3)
            Ra, Rb = np.eye(3), -np.eye(3)
            Rb[k, k] = 1.0
            R, t = po.se3_interpolate((Ra, ta), (Rb, tb), al)
            rows.append((np.concatenate([Ra.reshape(9), ta]), np.concatenate([Rb.reshape(9), tb]), al,
                         np.concatenate([R.reshape(9), t]), so.interpolate_mp((Ra, ta), (Rb, tb), al), len(ANGLES) - 1,
                         math.pi))
    A, B, alpha, ref, exact = (np.array([r[i] for r in rows]) for i in range(5))
    ai = np.array([r[5] for r in rows], dtype=np.int32)
    err = np.zeros((ai.max() + 1, 2))
    for a in sorted(set(ai.tolist())):
        e = np.abs(ref[ai == a] - exact[ai == a])
        err[a] = e[:, :9].max(), e[:, 9:].max()
    assert np.isfinite(err).all() and err.max() <= 1e-6, err.max()
    out.update(interp_A=A, interp_B=B, interp_alpha=alpha, interp_ref=ref, interp_exact=exact, interp_angle_id=ai,
               interp_theta=np.array([r[6] for r in rows]), interp_ref_err=err)
    print(f"interp rows {len(rows)}: planner_oracle.se3_interpolate vs exact, worst {err.max():.3e} "
          f"(angle id {int(err.max(axis=1).argmax())})")


def save(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    out = {}
    make_log(out)
    make_exp(out)
    make_interp(out)
    path = os.path.join(HERE, "se3_cases.npz")
    save(path, out)
    print(f"wrote se3_cases.npz, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
