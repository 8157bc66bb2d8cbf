"""The SE(3) logarithm and exponential on every device path, against the 50-digit
values of tests/golden/se3_cases.npz and, for inputs that only exist at run time (FK
outputs), se3_oracle.log6_accurate, which tests/test_se3.py holds to 8 eps of them.
Gates as in tests/test_se3.py (se3_oracle.gates); DESIGN.md "SE(3) log/exp accuracy by
path" has the table.  Nothing here needs mpmath.

  1  ikg_log6_batch f64 / f32 (E1, E2) over the fixture, and at B = 1 and B = 257
  2  ikg_se3_interpolate_batch (E3), numpy and device-tensor inputs
  3  the loops' log6_iter (E4, E5, E6) through the solve's own `err`: max_iters = 0 evaluates
     the pose error once at q0 and reports its norm (ikg_solve.hpp: the loop leaves at
     it >= max_iters before any update, nrm_out = sqrt(x)); the cube is placed so that the
     hand's error is a fixture row's
  4  the tracked angle: the same after 1, 2, kResync - 1, kResync, kResync + 1 updates
  5  the controller's orientation error (E1 inside ikg_frame_kinematics_batch)
"""
import math

import numpy as np
import pytest

import helpers
import se3_oracle as so
from ikgrasp import _lib

pytestmark = pytest.mark.gpu

EPS = so.EPS["f64"]
RESYNC64 = 128  # Trig<double>::kResync (ikg_device.hpp), as tests/test_gpu_resync_phase.py
CLAMP_HI = 25  # angle ids from here on: the clamp rows (make_se3_golden.py)
VARIANTS = {"pair-f64": ("f64", dict(variant=_lib.IKG_VARIANT_PAIR, ppw=32)),
            "quad-f64": ("f64", dict(variant=_lib.IKG_VARIANT_QUAD)),
            "pair-f32": ("f32", dict(variant=_lib.IKG_VARIANT_PAIR, ppw=32)),
            "packed-f32": ("f32", dict(variant=_lib.IKG_VARIANT_PACKED))}
# what the FK kernel and a loop's own FK may differ by: tests/test_gpu_parity.py holds the fp64 FK
# to 1e-13 of the oracle, 450 eps; the same count of fp32 roundings for the fp32 kernels (not a
# measured difference: it makes the fp32 checks here coarse)
FK_TOL = {"f64": 1e-13, "f32": 1e-13 * so.EPS["f32"] / so.EPS["f64"]}


@pytest.fixture(scope="module")
def fx():
    return so.load()


# ---------------------------------------------------------------- placements [n,12] in float64
def _mul(A, B):
    Ra, Rb = A[:, :9].reshape(-1, 3, 3), B[:, :9].reshape(-1, 3, 3)
    return np.concatenate([(Ra @ Rb).reshape(-1, 9), A[:, 9:] + np.einsum("nij,nj->ni", Ra, B[:, 9:])], axis=1)


def _inv(A):
    Rt = A[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    return np.concatenate([Rt.reshape(-1, 9), -np.einsum("nij,nj->ni", Rt, A[:, 9:])], axis=1)


def _hook(model, h, n, npt=np.float64):
    H = np.concatenate([np.asarray(model.hook_R[h], dtype=npt).reshape(9), np.asarray(model.hook_t[h], dtype=npt)])
    return np.broadcast_to(H.astype(np.float64), (n, 12))


def _rot(axis, theta):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(theta * np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)).as_matrix()


def _norm_gate(fx, E, dtype):
    """What |err - |log6_accurate(E)|| may be for the pose errors E [n,12]: the 2-norm of the
    rows' component gates -- 16x the reference restatement's own error on that very row, the
    floor, for fp64 the derived mid-band envelope -- plus the FK difference."""
    acc = so.log6_accurate(E)
    ref = np.array([so.log6_ref(e, dtype) for e in E], dtype=np.float64)
    th, pn = np.linalg.norm(acc[:, 3:], axis=1), np.linalg.norm(E[:, 9:], axis=1)
    eps = so.EPS[dtype]
    re = np.abs(ref - acc)
    g = np.empty((len(E), 6))
    g[:, :3] = np.maximum(16 * re[:, :3].max(axis=1), 4 * eps * np.maximum(1.0, pn))[:, None]
    g[:, 3:] = np.maximum(16 * re[:, 3:].max(axis=1), 4 * eps * np.maximum(1.0, th))[:, None]
    if dtype == "f64":
        g += so.envelope_gate(fx, th, pn, "derived")
    return np.linalg.norm(acc, axis=1), np.linalg.norm(g, axis=1) + FK_TOL[dtype] * np.maximum(1.0, pn), th


def _errors(model, hands, targets, npt=np.float64):
    """the two hands' pose errors hand^-1 (target hook) [n,2,12], composed in float64"""
    n = len(targets)
    return np.stack([_mul(_inv(hands[:, h].astype(np.float64)), _mul(targets, _hook(model, h, n, npt)))
                     for h in range(2)], axis=1)


# ---------------------------------------------------------------- 1: the public kernel
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_log6_batch_meets_its_gate(solver, fx, dtype):
    """IKSolver.log6 over the whole fixture (v of E1 in the mid band at the derived envelope), finite on the clamp rows, exact at
    R = 1, Pinocchio's signs at pi; B = 1 and B = 257 (one block and a row) give the batch's bits."""
    rows, g = so.gates(fx, dtype, envelope="derived" if dtype == "f64" else None)
    M = fx["M"][rows]
    raw = solver.log6(M, dtype)
    got = raw.astype(np.float64)
    assert got.shape == (len(rows), 6) and np.isfinite(got).all()
    ratio = np.abs(got - fx["exact"][rows]) / g
    th, ai = fx["theta"][rows], fx["angle_id"][rows]
    bands = {"taylor": (th < so.PREC3[dtype]) & (ai < CLAMP_HI), "mid": so.mid_band(th, dtype) & (ai < CLAMP_HI),
             "near_pi": (th >= so.NEAR_PI) & (ai < CLAMP_HI), "clamps": ai >= CLAMP_HI}
    err, pmax = np.abs(got - fx["exact"][rows]), np.maximum(1.0, np.linalg.norm(M[:, 9:], axis=1))[:, None]
    helpers.report(f"se3_gpu_log6_{dtype}", {b: {"w": float(ratio[s, 3:].max()), "v": float(ratio[s, :3].max()),
                                                 "abs_w": float(err[s, 3:].max()),
                                                 "abs_v_per_p": float((err[:, :3] / pmax)[s].max())}
                                             for b, s in bands.items()})
    bad = np.nonzero((ratio > 1).any(axis=1))[0]
    assert len(bad) == 0, ("rows", rows[bad][:8], "theta", th[bad][:8], "err/gate", ratio[bad][:8])
    ident, at_pi = ai == 0, ai == 24
    assert (got[ident, 3:] == 0).all() and np.array_equal(got[ident, :3], M[ident, 9:])
    assert np.array_equal(np.signbit(got[at_pi, 3:]), np.signbit(fx["ref"][rows][at_pi, 3:]))
    for a, b in ((300, 301), (100, 357)):  # B = 1; B = 257: one block of 256 and a row
        assert np.array_equal(solver.log6(M[a:b], dtype), raw[a:b], equal_nan=True)


def test_log6_batch_v_stated_envelope(solver, fx):
    """E1's v between kPrec3 and pi - 1e-2 against w's envelope times |p|,
    16 ref_err + 4 K_meas_v (eps / sin theta) |p| with K_meas_v = 4.55e3 measured on the numpy
    restatement of the form (tests/test_se3.py test_default_form_v_stated_envelope has the figures
    and why the constant is not O(1)); test_log6_batch_meets_its_gate holds the same rows to the
    tighter eps / sin^2(theta) |p|."""
    rows, g = so.gates(fx, "f64", envelope="stated")
    mid = so.mid_band(fx["theta"][rows]) & (fx["angle_id"][rows] < CLAMP_HI)
    ratio = (np.abs(solver.log6(fx["M"][rows], "f64") - fx["exact"][rows]) / g)[mid, :3].max(axis=1)
    th = fx["theta"][rows][mid]
    worst = {f"{t:.6g}": float(ratio[th == t].max()) for t in np.unique(th)}
    helpers.report("se3_gpu_log6_stated_v_envelope", worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------- 2: SE3.Interpolate
def test_se3_interpolate_meets_its_gate(solver, fx):
    """ikg_se3_interpolate_batch over the interpolation group: 16x the float64 restatement's
    error of the 50-digit placement (floor 4 eps on R, 4 eps max(1, |t|) on t); alpha = 0 returns A
    within the floor, alpha = 1 returns B within the gate; device tensors give the host arrays' bits."""
    import torch
    A, B, al = fx["interp_A"], fx["interp_B"], fx["interp_alpha"]
    got = solver.se3_interpolate(A, B, al)
    dev = solver.se3_interpolate(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, B, al)))
    assert np.array_equal(dev.cpu().numpy().view(np.int64), got.view(np.int64))
    re = fx["interp_ref_err"][fx["interp_angle_id"]]
    tn = np.linalg.norm(fx["interp_exact"][:, 9:], axis=1)
    gR, gt = np.maximum(16 * re[:, 0], 4 * EPS), np.maximum(16 * re[:, 1], 4 * EPS * np.maximum(1.0, tn))
    err = np.abs(got - fx["interp_exact"])
    rR, rt = err[:, :9].max(axis=1) / gR, err[:, 9:].max(axis=1) / gt
    helpers.report("se3_gpu_interpolate", {"R": float(rR.max()), "t": float(rt.max())})
    assert rR.max() <= 1.0 and rt.max() <= 1.0, (np.nonzero((rR > 1) | (rt > 1))[0][:8], rR.max(), rt.max())
    a0, a1 = al == 0.0, al == 1.0
    assert (np.abs(got[a0] - A[a0]).max(axis=1) <= 4 * EPS * np.maximum(1.0, np.linalg.norm(A[a0, 9:], axis=1))).all()
    e1 = np.abs(got[a1] - B[a1])
    assert (e1[:, :9].max(axis=1) <= gR[a1]).all() and (e1[:, 9:].max(axis=1) <= gt[a1]).all()


# ---------------------------------------------------------------- 3: the loops, at q0
def _subset(fx, dtype):
    """64 fixture rows of `dtype`: per angle the zero-component and the random class, and the
    coordinate class at every edge (0, kPrec3 -+, pi/2 -+, pi - 1e-2 -+, near pi, pi)"""
    rows = np.nonzero((fx["dtype"] == (0 if dtype == "f64" else 1)) & (fx["angle_id"] < CLAMP_HI))[0]
    ai, cls = fx["angle_id"][rows], fx["axis_class"][rows]
    no_coord = {1, 2, 3, 9, 10, 12, 14, 15, 17, 18}
    pick = []
    for a in range(CLAMP_HI):
        for c in range(3):
            s = rows[(ai == a) & (cls == c)]
            if len(s) and not (c == 0 and a in no_coord):
                pick.append(s[(a + c) % len(s)])  # another |p| from angle to angle
    assert len(pick) == 64
    return np.array(pick)


@pytest.fixture(scope="module")
def bases(solver):
    """Yawed cube placements with the arms on them: IK solutions to 1e-11, computed once"""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(192, seed=12, yaw=np.pi)
    sol = solver.solve(tg, np.zeros(solver.nq), eps=1e-11, max_iters=6000, **VARIANTS["pair-f64"][1])
    ok = np.nonzero(sol.converged)[0]
    assert len(ok) >= 25, len(ok)
    return tg[ok], sol.q[ok]


def _check_err(solver, fx, name, targets, q0, what):
    """solve(max_iters = 0): both hands' err against |log6_accurate| of the error composed from
    the same dtype's solver.fk(q0)"""
    dtype, kw = VARIANTS[name]
    npt = np.float64 if dtype == "f64" else np.float32
    tg, q = targets.astype(npt), q0.astype(npt)
    sol = solver.solve(tg, q, dtype=dtype, max_iters=0, **kw)
    assert not sol.converged.any() and (sol.iters == 0).all()
    E = _errors(solver.model, solver.fk(q, dtype), tg.astype(np.float64), npt)
    worst = {}
    for h in range(2):
        want, gate, th = _norm_gate(fx, E[:, h], dtype)
        ratio = np.abs(sol.err[:, h].astype(np.float64) - want) / gate
        worst[f"hand{h}"] = float(ratio.max())
        assert ratio.max() <= 1.0, (name, what, "hand", h, "row", int(ratio.argmax()), "theta", th[ratio.argmax()],
                                    "err", sol.err[ratio.argmax(), h], "want", want[ratio.argmax()], "gate", gate[ratio.argmax()])
    helpers.report(f"se3_gpu_err_{name}_{what}", worst)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_loop_error_at_fixture_rows_general(solver, fx, name):
    """A general batch: target = FK_hand(q0) M hook^-1 puts hand (row % 2)'s error at the fixture
    row's M for 64 seeds q0 (random within the limits); the other hand's is checked the same way."""
    from ikgrasp.workload import random_seeds
    dtype = VARIANTS[name][0]
    rows = _subset(fx, dtype)
    q0 = random_seeds(solver.model, len(rows), seed=41)
    if dtype == "f32":
        q0 = q0.astype(np.float32).astype(np.float64)
    hands = solver.fk(q0).astype(np.float64)
    which = np.arange(len(rows)) % 2
    M = fx["M"][rows].copy()
    # within 1e3 eps_T of pi (fp64: pi itself; fp32: from pi - 1e-6) with p = 0: once composed with the FK
    # the skew part is rounding noise, each component of w takes its sign from it, and |v| depends on
    # those signs (|w| does not)
    M[math.pi - fx["theta"][rows] < 1e3 * so.EPS[dtype], 9:] = 0.0
    tg = np.empty((len(rows), 12))
    for h in range(2):
        s = which == h
        tg[s] = _mul(_mul(hands[s, h], M[s]), _inv(_hook(solver.model, h, int(s.sum()))))
    _check_err(solver, fx, name, tg, q0, "general")


def _yaw_batch(fx, bases):
    """the bases' cubes yawed on by each of the fixture's angles and shifted by 0, 1e-3, 1 or 10"""
    tg0, q = bases
    th = np.unique(fx["theta"][fx["angle_id"] < CLAMP_HI])
    n = len(th)
    rng = np.random.default_rng(43)
    tg = tg0[:n].copy()
    psi = np.arctan2(tg[:, 3], tg[:, 0]) + th
    tg[:, 0], tg[:, 1], tg[:, 3], tg[:, 4] = np.cos(psi), -np.sin(psi), np.sin(psi), np.cos(psi)
    u = rng.normal(size=(n, 3))
    tg[:, 9:] += u / np.linalg.norm(u, axis=1, keepdims=True) * np.array([0.0, 1e-3, 1.0, 10.0])[np.arange(n) % 4][:, None]
    return tg, q[:n]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_loop_error_at_fixture_angles_z_aligned(solver, fx, bases, name):
    """A yaw-only batch (every hook target a rotation about z: the pair kernel runs its
    z-aligned loop): the cube yawed by each fixture angle away from a placement the arms are on
    (IK to 1e-11), so both hands' errors turn by that angle."""
    tg, q0 = _yaw_batch(fx, bases)
    assert (tg[:, [2, 5, 6, 7]] == 0).all() and (tg[:, 8] == 1).all()
    if VARIANTS[name][0] == "f32":
        q0 = q0.astype(np.float32).astype(np.float64)
    _check_err(solver, fx, name, tg, q0, "z_aligned")


# ---------------------------------------------------------------- 4: the tracked angle
THETA0 = (3e-4, 3e-3, 1e-2, math.pi - 2e-2)


def _tracked_batches(solver, bases):
    """(general, yaw-only): per start angle four problems whose hands' errors turn by it at q0.
    General: the cube turned about a random axis through hand 0's hook and shifted by 1e-2;
    yaw-only: yawed and shifted."""
    tg0, q = bases
    rng = np.random.default_rng(44)
    n = 4 * len(THETA0)
    th = np.repeat(THETA0, 4)
    q0 = q[:n]
    hands = solver.fk(q0).astype(np.float64)
    u = rng.normal(size=(n, 3))
    M = np.array([np.concatenate([_rot(rng.normal(size=3), t).reshape(9), 1e-2 * x / np.linalg.norm(x)])
                  for t, x in zip(th, u)])
    general = _mul(_mul(hands[:, 0], M), _inv(_hook(solver.model, 0, n)))
    yaw = tg0[:n].copy()
    psi = np.arctan2(yaw[:, 3], yaw[:, 0]) + th
    yaw[:, 0], yaw[:, 1], yaw[:, 3], yaw[:, 4] = np.cos(psi), -np.sin(psi), np.sin(psi), np.cos(psi)
    yaw[:, 9:] += 1e-2 * u / np.linalg.norm(u, axis=1, keepdims=True)
    return {"general": general, "z_aligned": yaw}, q0, th


@pytest.mark.parametrize("max_iters", [1, 2, RESYNC64 - 1, RESYNC64, RESYNC64 + 1])
@pytest.mark.parametrize("name,what", [("pair-f64", "general"), ("pair-f64", "z_aligned"), ("quad-f64", "general")])
def test_tracked_angle_reported_error(solver, fx, bases, name, what, max_iters):
    """eps = 1e-12 so that nothing passes: the loop leaves at max_iters and reports the error of
    the iterate it returns, whose angle was carried through max_iters % kResync increments.  It
    equals |log6_accurate| at solver.fk(q_out) within the E4 gate and the FK term."""
    batches, q0, th0 = _tracked_batches(solver, bases)
    tg = batches[what]
    sol = solver.solve(tg, q0, eps=1e-12, max_iters=max_iters, **VARIANTS[name][1])
    assert not sol.converged.any() and (sol.iters == max_iters).all()
    E = _errors(solver.model, solver.fk(sol.q), tg)
    worst = {}
    for h in range(2):
        want, gate, th = _norm_gate(fx, E[:, h], "f64")
        ratio = np.abs(sol.err[:, h] - want) / gate
        worst[f"hand{h}"] = float(ratio.max())
        assert ratio.max() <= 1.0, (name, what, max_iters, "hand", h, "row", int(ratio.argmax()), th[ratio.argmax()],
                                    sol.err[ratio.argmax(), h], want[ratio.argmax()], gate[ratio.argmax()])
    helpers.report(f"se3_gpu_tracked_{name}_{what}_{max_iters}", worst)


# ---------------------------------------------------------------- 5: the controller's orientation error
def test_controller_orientation_error(solver, fx):
    """frame_kinematics' err: its rotation part is log3(R_des R^T) by log6<double>.  q_des turns
    each arm's last wrist joint by the fixture's angles (q at -theta/2, q_des at +theta/2), so
    R_des R^T turns by theta about the wrist axis; the two frames come from the same kernel.  The
    other joints are random within their limits: a wrist axis in general position (on a grasp
    it lies along a world axis to 1e-11, and near pi such a component is the root of a rounding
    residue, the fixture's zero-component class).  Gate: E1's on w (16x the reference's own error,
    on the row and on the fixture's random-axis bucket of that angle; floor 4 eps max(1, theta);
    envelope 4 K_meas eps / sin theta); no FK term, the frames being the kernel's own."""
    from ikgrasp.workload import random_seeds
    sel = (fx["angle_id"] < CLAMP_HI) & (fx["dtype"] == 0) & (fx["axis_class"] == 2)
    th, first = np.unique(fx["theta"][sel], return_index=True)
    bucket_err = fx["ref_err"][fx["bucket"][sel][first], 0]
    assert {2e-4, 1e-3, math.pi - 1e-3} <= set(th.tolist())
    n = len(th)
    q = random_seeds(solver.model, n, seed=45)
    qd = q.copy()
    for h in range(2):
        j = int(solver.model.arm_q[h][-1])
        q[:, j], qd[:, j] = -th / 2, th / 2
    res = solver.frame_kinematics(q, q_des=qd, outputs=("placement", "err"))
    des = solver.frame_kinematics(qd, outputs=("placement",))["placement"]
    worst = {}
    for h in range(2):
        R, Rd = res["placement"][:, h, :9].reshape(-1, 3, 3), des[:, h, :9].reshape(-1, 3, 3)
        E = np.concatenate([(Rd @ R.transpose(0, 2, 1)).reshape(-1, 9), np.zeros((n, 3))], axis=1)
        acc = so.log6_accurate(E)[:, 3:]
        ref = np.array([so.log6_ref(e)[3:] for e in E])
        ang = np.linalg.norm(acc, axis=1)
        assert np.abs(ang - th).max() <= 1e-9
        gate = (np.maximum(16 * np.maximum(np.abs(ref - acc).max(axis=1), bucket_err), 4 * EPS * np.maximum(1.0, ang))
                + so.envelope_gate(fx, ang, np.zeros(n))[:, 3])
        ratio = np.abs(res["err"][:, 6 * h + 3:6 * h + 6] - acc).max(axis=1) / gate
        worst[f"hand{h}"] = float(ratio.max())
        assert ratio.max() <= 1.0, ("hand", h, "theta", ang[ratio.argmax()], ratio.max())
    helpers.report("se3_gpu_controller_err", worst)
