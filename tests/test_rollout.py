"""Forward dynamics, Bezier desired state and the closed-loop rollout on the CPU:
the host emulation of the kernels' arithmetic (ikg_emu_forward_dynamics,
ikg_emu_bezier, ikg_emu_control_rollout) against tests/golden/rollout_cases.npz,
whose bounds are measured (make_rollout_golden.py: 20 x the float64
restatement's error against the 50-digit evaluation), the oracle's own
consistency, the Python layer (`ikgrasp.control.Simulation`, `load_trajectory`)
and the C-ABI argument checks."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import dynamics_oracle as do
import rollout_cases as rc
import rollout_oracle as ro
from ikgrasp import _lib, control


@pytest.fixture(scope="module")
def d():
    return rc.load()


@pytest.fixture(scope="module")
def dc():
    return dict(np.load(rc.os.path.join(rc.GOLDEN, "dynamics_cases.npz")))


@pytest.fixture(scope="module")
def solvers():
    return {name: rc.EmuSolver(m, bi) for name, (m, bi) in rc.models().items()}


@pytest.fixture(scope="module")
def nextage_rollouts(solvers, d):
    """The 16 starts x 32 ticks of the fixture, emulated once."""
    return rc.run_rollouts(solvers["nextage"], d, "nextage", 32)


# ---------------------------------------------------------------- Bezier
def test_bezier_matches_fixture(solvers, d):
    rc.check_bezier(solvers["nextage"], d)


def test_bezier_oracle_is_the_bernstein_sum(d):
    """The Horner restatement against the definition sum_i C(n,i) u^i (1-u)^(n-i) P_i, in 50 digits."""
    import mpmath
    cq, _ = rc.traj_curves(d, 1, False)
    P, n = cq[0], len(cq[0]) - 1
    for t in (0.0, 4.2, 15.0):
        u = mpmath.mpf(t) / mpmath.mpf(15)
        want = [sum(mpmath.binomial(n, i) * u ** i * (1 - u) ** (n - i) * mpmath.mpf(float(P[i, j])) for i in range(n + 1))
                for j in range(P.shape[1])]
        got = ro.bezier(do.MP, cq, t)
        assert max(abs(a - b) for a, b in zip(got, want)) < mpmath.mpf(10) ** -45


def test_bezier_two_points_and_errors(solvers):
    s = solvers["nextage"]
    P = np.array([[1.0, -2.0, 0.5], [7.0, 7.0, 7.0]])
    out = s.bezier(P, 1.0, 3.0, 0.25, [1.0, 2.0, 3.0])
    assert np.array_equal(out, np.tile(0.25 * P[0], (3, 1)))  # the reference's size_ == 1 branch
    P3 = np.vstack([P, [[0.0, 1.0, 2.0]]])
    for bad in (dict(points=P[:1]), dict(t_max=1.0), dict(t_max=0.5), dict(points=np.zeros((65, 3))),
                dict(times=[0.999]), dict(times=[3.0001])):
        a = dict(points=P3, t_min=1.0, t_max=3.0, mult=1.0, times=[2.0])
        a.update(bad)
        with pytest.raises(_lib.IkgError):
            s.bezier(**a)
    assert s.bezier(np.zeros((64, 3)), 0.0, 1.0, 1.0, [0.5]).shape == (1, 3)


def test_curve_class_and_load_trajectory(tmp_path, d, solvers):
    """ikgrasp.control.Curve / load_trajectory: the reference's JSON layout; every curve keeps the file's mult_t."""
    cq, cvfile = rc.traj_curves(d, 1, True)
    _, cvder = rc.traj_curves(d, 1, False)
    path = tmp_path / "trajectory.json"
    path.write_text(json.dumps({"q_control_points": cq[0].tolist(), "vq_control_points": cvfile[0].tolist(),
                                "vvq_control_points": np.zeros((len(cq[0]) - 2, 15)).tolist(), "t_min": cq[1], "t_max": cq[2],
                                "mult_t": cq[3]}))
    q_of_t, vq_of_t, vvq_of_t = control.load_trajectory(str(path))
    assert (vq_of_t.T_min_, vq_of_t.T_max_, vq_of_t.mult_T_) == (cq[1], cq[2], cq[3])  # unscaled, as the reference loads it
    assert np.array_equal(np.array(q_of_t.control_points_), cq[0]) and len(vvq_of_t.control_points_) == len(cq[0]) - 2
    der = q_of_t.derivative(1)
    assert np.array_equal(np.array(der.control_points_), cvder[0]) and der.mult_T_ == cvder[3]
    for t in (0.0, 0.07, 9.3, 15.0):
        assert np.array_equal(q_of_t(t), ro.bezier(do.F64, cq, t))
        assert np.array_equal(der(t), ro.bezier(do.F64, cvder, t))
    with pytest.raises(ValueError):
        q_of_t(15.01)
    pts, t_min, t_max, mult = _lib.curve(der)
    assert pts.shape == (len(cq[0]) - 1, 15) and (t_min, t_max, mult) == (0.0, 15.0, der.mult_T_)


# ---------------------------------------------------------------- forward dynamics
def test_forward_dynamics_within_measured_bound(solvers, d, dc):
    """The 96 states of dynamics_cases.npz with their tau, against 50 digits.
    Bound: tol_fd = 20 x the float64 restatement's error, 4.68e-14 of max|qdd|.
    Forward dynamics forms M about each joint's own origin (ikg_dynamics.hpp):
    with the dynamics kernel's M, exact to 3.6e-16 of max|M| but not relative
    to its small wrist rows, the same solve is at 1.8e-13 (cond(M) up to 1.4e4,
    |qdd| up to 1.7e5 on the stretched-elbow states)."""
    rc.check_forward_dynamics(solvers["nextage"], dc["q"], dc["v"], dc["tau"], d["fd_qdd_mp"], float(d["tol_fd"]),
                              "nextage")


def test_forward_dynamics_satisfies_its_equation(solvers, d, dc):
    rc.check_forward_dynamics_equation(solvers["nextage"], dc["q"], dc["v"], dc["tau"], float(d["tol_fd"]), "nextage")


def test_forward_dynamics_of_the_32_joint_model(solvers, d):
    s = solvers["mixed"]
    rc.check_forward_dynamics(s, d["mixed_fd_q"], d["mixed_fd_v"], d["mixed_fd_tau"], d["mixed_fd_qdd_mp"],
                              float(d["mixed_tol_fd"]), "mixed_axes")
    rc.check_forward_dynamics_equation(s, d["mixed_fd_q"], d["mixed_fd_v"], d["mixed_fd_tau"], float(d["mixed_tol_fd"]),
                                       "mixed_axes")


def test_forward_dynamics_oracle_formulations_agree(d, dc):
    m, bi = rc.models()["nextage"]
    t = do.Tree(do.F64, m, bi)
    for i in (0, 40, 90):
        a = ro.forward_dynamics(t, dc["q"][i], dc["v"][i], dc["tau"][i])
        b = ro.forward_dynamics(t, dc["q"][i], dc["v"][i], dc["tau"][i], inverse=True)
        np.testing.assert_allclose(a, b, rtol=0, atol=float(d["tol_fd"]) * np.abs(d["fd_qdd_mp"]).max())
        np.testing.assert_allclose(do.rnea(t, dc["q"][i], dc["v"][i], a), dc["tau"][i], rtol=0,
                                   atol=1e-9 * np.abs(dc["tau"][i]).max())


# ---------------------------------------------------------------- rollouts
def test_rollouts_within_per_tick_bounds(nextage_rollouts, d):
    rc.check_rollouts(nextage_rollouts, d, "nextage", "emulator")


@pytest.mark.parametrize("name,ticks", [("tilted", 16), ("mixed", 8)])
def test_other_models_within_per_tick_bounds(solvers, d, name, ticks):
    rc.check_rollouts(rc.run_rollouts(solvers[name], d, name, ticks), d, name, "emulator")


def test_oracle_tick_variants_move_outside_the_bounds(d):
    """The checks can see an integrator or clock fault: the float64 oracle with
    explicit Euler, or without the clock advance, leaves the per-tick bounds."""
    m, bi = rc.models()["nextage"]
    t = do.Tree(do.F64, m, bi)
    cq, cv = rc.traj_curves(d, 1, False)
    q, v, tt = d["ro_q0"][0], d["ro_v0"][0], float(d["ro_t0"][0])
    assert not d["ro_alt"][0] and d["ro_traj"][0] == 1 and not d["ro_vfile"][0]
    qe, ve, te = q, v, tt
    qs, vs = q, v
    for k in range(4):
        qe, ve, te, _ = ro.tick(t, qe, ve, te, cq, cv, euler="explicit")
        qs, vs, _, _ = ro.tick(t, qs, vs, tt, cq, cv)  # the clock stands still
    ref, tol = d["ro_q_mp"], d["tol_q"]
    assert np.abs(qe - ref[0, 3]).max() > tol[3] * np.abs(ref).max()
    assert np.abs(qs - ref[0, 3]).max() > tol[3] * np.abs(ref).max()


def test_clamp_holds_the_end_point(solvers, d):
    """Past t_max the desired state is the curve's end point: a start beyond the
    range equals, bit for bit, a start at t_max and a rollout on constant curves
    at the end points; the fixture's last start crosses t_max on the way."""
    s = solvers["nextage"]
    cq, cv = rc.traj_curves(d, 1, False)
    q0, v0 = d["ro_q0"][3:4], d["ro_v0"][3:4]
    assert d["ro_t0"][3] < cq[2] < d["ro_t0"][3] + 32 * 1e-2
    kw = dict(ticks=6, record_every=1, outputs=rc.HIST + ("t",))
    a = s.rollout(q0, v0, (cq, cv), t0=[cq[2] + 5.0], **kw)
    b = s.rollout(q0, v0, (cq, cv), t0=[cq[2]], **kw)
    end = lambda c: (np.vstack([c[3] * c[0][-1:], c[3] * c[0][-1:]]), 0.0, 1.0, 1.0)
    c = s.rollout(q0, v0, (end(cq), end(cv)), t0=[0.0], **kw)
    for k in rc.HIST:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert a["t"][0] == pytest.approx(cq[2] + 5.06, rel=1e-14) and b["t"][0] > cq[2]  # the clock itself is not clamped


def test_inputs_untouched_and_record_every(solvers, d, nextage_rollouts):
    s = solvers["nextage"]
    rows, trajs, gains = rc.groups(d, "nextage")[0]
    q0, v0, t0 = d["ro_q0"][rows].copy(), d["ro_v0"][rows].copy(), d["ro_t0"][rows].copy()
    keep = (q0.copy(), v0.copy(), t0.copy())
    full = {k: nextage_rollouts[k][rows] for k in rc.OUT}
    r0 = s.rollout(q0, v0, trajs, t0=t0, ticks=32, **gains)
    assert set(r0) == {"q", "v", "t"}
    assert np.array_equal(r0["q"], full["q"][:, -1]) and np.array_equal(r0["v"], full["v"][:, -1])
    tt = t0.copy()
    for _ in range(32):
        tt = tt + 1e-2
    assert np.array_equal(r0["t"], tt)  # one float64 add per tick
    r4 = s.rollout(q0, v0, trajs, t0=t0, ticks=30, record_every=4, outputs=rc.HIST + ("q",), **gains)
    assert r4["q_hist"].shape == (len(rows), 7, 15)
    for k in rc.OUT:
        assert np.array_equal(r4[k + "_hist"], full[k][:, 3:28:4]), k
    assert np.array_equal(r4["q"], full["q"][:, 29])
    for a, b in zip((q0, v0, t0), keep):
        assert np.array_equal(a, b)
    z = s.rollout(q0, v0, trajs, t0=None, ticks=0)
    assert np.array_equal(z["q"], q0) and np.array_equal(z["v"], v0) and np.all(z["t"] == trajs[0][1])
    with pytest.raises(_lib.IkgError):
        s.rollout(q0, v0, trajs, ticks=4, record_every=0, outputs=("q_hist",))


def test_simulation_loop_agrees_with_rollout(solvers, d, nextage_rollouts):
    """The reference's loop (control.py:461-463) with `Simulation` as the
    simulator and `controllaw` unmodified, 8 ticks, against the rollout's
    records to the per-tick bounds."""
    s = solvers["nextage"]
    i = 0
    assert not d["ro_alt"][i]
    cq, cv = rc.traj_curves(d, int(d["ro_traj"][i]), bool(d["ro_vfile"][i]))
    trajs = (control.Curve(cq[0], cq[1], cq[2], cq[3]), control.Curve(cv[0], cv[1], cv[2], cv[3]))

    class Robot:
        solver = s

    sim = control.Simulation(Robot, dt=1e-3)
    sim.setqsim(d["ro_q0"][i], d["ro_v0"][i])
    tcur, DT = float(d["ro_t0"][i]), 0.01
    for k in range(8):
        control.controllaw(sim, Robot, trajs, tcur, None)
        tcur += DT
        q, v = sim.getpybulletstate()
        for name, x in (("q", q), ("v", v)):
            ref = d[f"ro_{name}_mp"]
            assert np.abs(x - ref[i, k]).max() <= d["tol_" + name][k] * np.abs(ref).max(), (name, k)
            assert np.abs(x - nextage_rollouts[name][i, k]).max() <= 2 * d["tol_" + name][k] * np.abs(ref).max()


# ---------------------------------------------------------------- C-ABI
def test_new_entries_reject_bad_arguments():
    from ikgrasp.model import load_nextage, load_nextage_inertia
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ikg_model_create(C.byref(_lib.model_desc(load_nextage())), C.byref(h)) == 0
    msg = lambda: lib.ikg_last_error().decode()
    HOST = _lib.IKG_FLAG_HOST_POINTERS
    buf = np.zeros(15)
    p = buf.ctypes.data
    P = np.zeros((3, 15))
    bq, _k1 = _lib.bezier_desc((P, 0.0, 1.0, 1.0), 15)
    prm, out = _lib.rollout_params(4), _lib.RolloutOut()
    roll = lambda q0=p, bq=bq, bv=bq, prm=prm, out=out, B=1, model=h: lib.ikg_control_rollout(
        model, 0, q0, p, None, B, C.byref(bq), C.byref(bv), C.byref(prm) if prm else None,
        C.byref(out) if out else None, None, HOST)
    assert roll() == -1 and "inertia" in msg()
    assert lib.ikg_forward_dynamics_batch(h, 0, p, p, p, 1, p, None, HOST) == -1 and "inertia" in msg()
    assert lib.ikg_model_set_inertia(h, C.byref(_lib.inertia_desc(load_nextage_inertia()))) == 0
    assert roll(model=None) == -1 and roll(prm=None) == -1 and roll(out=None) == -1 and roll(B=-1) == -1
    assert roll(q0=None) == -1 and "q0" in msg()
    for bad in ((P[:1], 0.0, 1.0, 1.0), (P, 1.0, 1.0, 1.0), (np.zeros((65, 15)), 0.0, 1.0, 1.0),
                (P, 0.0, 1.0, float("nan"))):
        b, _k2 = _lib.bezier_desc(bad, 15)
        assert roll(bq=b) == -1 and "q_curve" in msg()
        assert roll(bv=b) == -1 and "v_curve" in msg()
    nanq = buf.copy()
    nanq[3] = np.inf
    assert roll(q0=nanq.ctypes.data) == -1 and "not finite" in msg()
    hist = _lib.RolloutOut(None, None, None, p, None, None)
    assert roll(out=hist) == -1 and "record_every" in msg()
    assert roll(prm=_lib.rollout_params(-1)) == -1
    assert lib.ikg_forward_dynamics_batch(h, 0, p, p, None, 1, p, None, HOST) == -1 and "required" in msg()
    assert lib.ikg_forward_dynamics_batch(h, 0, nanq.ctypes.data, p, p, 1, p, None, HOST) == -1 and "not finite" in msg()
    assert lib.ikg_forward_dynamics_batch(h, 0, p, p, p, -1, p, None, HOST) == -1
    t = np.array([0.5, 1.5])
    bez = lambda n=3, dim=15, t_max=1.0, K=1: lib.ikg_bezier_eval_batch(0, P.ctypes.data, n, dim, 0.0, t_max, 1.0,
                                                                       t.ctypes.data, K, p, None, HOST)
    assert bez(n=1) == -1 and bez(n=65) == -1 and bez(t_max=0.0) == -1 and bez(dim=0) == -1 and bez(dim=33) == -1
    assert bez(K=2) == -1 and "outside" in msg()
    d0 = _lib.RolloutParams()
    lib.ikg_rollout_params_default(C.byref(d0))
    assert (d0.dt_sim, d0.dt_traj, d0.ticks, d0.record_every) == (1e-3, 1e-2, 0, 0)
    assert d0.control.Kp == 7000.0 and d0.control.fc_bias[1] == -200.0
    lib.ikg_model_destroy(h)


def test_ctypes_structures_match_the_header(tmp_path):
    """Sizes and field offsets of the rollout structures in ikgrasp/_lib.py from a C
    probe (tests/abi_probe_rollout.c) compiled against include/ikgrasp.h."""
    from conftest import ROOT
    exe = str(tmp_path / "abi_probe_rollout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "abi_probe_rollout.c")], check=True)
    rows = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    structs = {"ikg_bezier": _lib.Bezier, "ikg_rollout_params": _lib.RolloutParams, "ikg_rollout_out": _lib.RolloutOut}
    seen = set()
    for name, field, off, size in rows:
        cls = structs[name]
        if field == "sizeof":
            assert C.sizeof(cls) == int(size), name
        else:
            f = getattr(cls, field)
            assert (f.offset, f.size) == (int(off), int(size)), (name, field)
        seen.add((name, field))
    for name, cls in structs.items():
        for field, _ in cls._fields_:
            assert (name, field) in seen, (name, field)
