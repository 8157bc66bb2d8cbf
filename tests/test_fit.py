"""The Bezier trajectory fit (ikg_bezier_fit_batch, the reference's maketraj) and
the per-state rollout (ikg_control_rollout_curves) on the CPU: the host
emulation of the kernels' arithmetic (ikg_emu_bezier_fit,
ikg_emu_control_rollout_curves) against tests/golden/fit_cases.npz, whose bounds
are measured (make_fit_golden.py: 20 x the float64 restatement's error against
the 50-digit minimiser), the reference's own maketraj results stored there, the
Python layer (`ikgrasp.control.maketraj`, `maketraj_batch`, `save_trajectory`)
and the C-ABI argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import fit_oracle as fo
import rollout_cases as rc
from ikgrasp import _lib, control


@pytest.fixture(scope="module")
def d():
    return fc.load()


@pytest.fixture(scope="module")
def fitter():
    return fc.EmuFit()


@pytest.fixture(scope="module")
def rd():
    return rc.load()


@pytest.fixture(scope="module")
def nextage():
    m, bi = rc.models()["nextage"]
    return rc.EmuSolver(m, bi)


# ---------------------------------------------------------------- the fit against 50 digits
@pytest.mark.parametrize("name", list(fc.CASES))
def test_fit_within_measured_bounds(fitter, d, name):
    r = fc.check_case(fitter.bezier_fit, d, name, "emulator")
    fc.check_derivatives(r, fc.CASES[name][2])


def test_oracles_agree_and_see_the_normal_equations(d):
    """The float64 restatement is inside its own bound / 20 by construction; the
    normal equations with a Cholesky factor, the shortcut, leave the
    control-point bound of the worst-conditioned case by orders of magnitude, so
    the check can see a solver of that accuracy."""
    name = "n17"
    n, dim, deg, ridge, T, _ = fc.CASES[name]
    q0, q1, y = fc.inputs(d, name)
    P64 = fo.fit_f64(q0, q1, y, T, deg, ridge)
    eP, eC, _ = fc.errors(d, name, P64, fo.cost_f64(P64, y, T))
    assert eP * fc.FACTOR <= float(d[name + "_tol_P"]) * (1 + 1e-12)
    _, u = fo.times(n, T)
    A = fo.bernstein(u, deg)
    X0 = fo.start_points(q0, q1, deg)
    Af = A[1:-1, 3:deg - 2]  # the end rows of A_f are zero
    L = np.linalg.cholesky(Af.T @ Af)
    delta = np.linalg.solve(L.T, np.linalg.solve(L, Af.T @ (y - A @ X0)[1:-1]))
    Pn = X0.copy()
    Pn[3:deg - 2] += delta
    eN, _, _ = fc.errors(d, name, Pn, 0.0)
    print(f"normal equations: control points {eN:.2e} of max|P| (bound {float(d[name + '_tol_P']):.2e})")
    assert eN > 100 * float(d[name + "_tol_P"])


def test_degree_6_is_the_closed_form(fitter, d):
    """One free control point: delta = sum a_k r_k / (sum a_k^2 + ridge) per joint."""
    name = "d6"
    n, dim, deg, ridge, T, _ = fc.CASES[name]
    q0, q1, y = fc.inputs(d, name)
    r = fc.fit_case(fitter.bezier_fit, d, name)
    _, u = fo.times(n, T)
    A = fo.bernstein(u, deg)
    X0 = fo.start_points(q0, q1, deg)
    a, res = A[:, 3], y - A @ X0
    want = X0[3] + (a @ res) / (a @ a + ridge)
    assert np.abs(r["points"][3] - want).max() <= 16 * fc.EPS * np.abs(want).max()


def test_ragged_batch_equals_one_path_per_call(fitter, d):
    fc.check_ragged(fitter.bezier_fit, d)


@pytest.mark.parametrize("name", fc.REFERENCE)
def test_not_above_the_references_cost(fitter, d, name):
    fc.check_reference(fitter.bezier_fit, d, name)


def test_count_out_of_range_is_refused_per_path(fitter, d):
    """Counts 1, 257 and (ridge 0) 16 among good paths: status 1, cost NaN,
    points untouched, neighbours as solved alone."""
    q0, q1, y = fc.inputs(d, "n40")
    long = np.vstack([d["n256_y"], d["n256_y"][:1]])
    paths = [y, y[:1], y, long, y[:16], y]
    yy, off = fc.pack(paths)
    r = fitter.bezier_fit(np.tile(q0, (6, 1)), np.tile(q1, (6, 1)), yy, off, total_time=1.0, degree=20, ridge=0.0)
    assert list(r["status"]) == [0, 1, 0, 1, 1, 0]
    one = fitter.bezier_fit(q0[None], q1[None], y, np.array([0, 40]), total_time=1.0, degree=20, ridge=0.0)
    for p in (0, 2, 5):
        assert np.array_equal(r["points"][p], one["points"][0]) and r["cost"][p] == one["cost"][0]
    for p in (1, 3, 4):
        assert np.isnan(r["cost"][p]) and np.all(r["points"][p] == -7.0)  # EmuFit's fill value


# ---------------------------------------------------------------- Python layer
def test_maketraj_is_a_drop_in(fitter, d):
    q0, q1, y = fc.inputs(d, "n40w")
    trajs, flag = control.maketraj(q0, q1, y, 15.0, solver=fitter)
    assert isinstance(trajs, list) and len(trajs) == 3 and flag is True
    q_of_t, vq_of_t, vvq_of_t = trajs
    assert all(isinstance(c, control.Curve) for c in trajs)
    assert (q_of_t.degree_, vq_of_t.degree_, vvq_of_t.degree_) == (20, 19, 18)
    assert (q_of_t.T_min_, q_of_t.T_max_, q_of_t.mult_T_) == (0.0, 15.0, 1.0)
    for got, want in ((vq_of_t, q_of_t.derivative(1)), (vvq_of_t, q_of_t.derivative(2))):
        assert np.array_equal(np.array(got.control_points_), np.array(want.control_points_))
        assert got.mult_T_ == want.mult_T_
    assert vq_of_t.mult_T_ == 1.0 / 15.0
    assert np.array_equal(q_of_t(0.0), q0) and np.array_equal(q_of_t(15.0), q1)
    assert np.all(vq_of_t(0.0) == 0) and np.all(vvq_of_t(15.0) == 0)  # the reference's end constraints
    r = fc.fit_case(fitter.bezier_fit, d, "n40w")
    assert np.array_equal(np.array(q_of_t.control_points_), r["points"])
    # the zigzag: a cost above 0.15 gives the reference's False
    _, flag = control.maketraj(*fc.inputs(d, "zig"), 1.0, solver=fitter)
    assert flag is False and float(d["zig_cost"]) > 1.0
    # a short path takes the documented ridge; above 256 points raise
    trajs, flag = control.maketraj(*fc.inputs(d, "n16r"), 15.0, solver=fitter)
    assert np.array_equal(np.array(trajs[0].control_points_), fc.fit_case(fitter.bezier_fit, d, "n16r")["points"])
    with pytest.raises(ValueError):
        control.maketraj(q0, q1, np.zeros((257, 15)), 1.0, solver=fitter)
    with pytest.raises(ValueError):
        control.maketraj(q0, q1, np.zeros((30, 14)), 1.0, solver=fitter)


def test_maketraj_batch_and_trajectory_file(fitter, d, tmp_path):
    names = ("n17", "n40", "n18")
    q0s = [d[k + "_q0"] for k in names]
    q1s = [d[k + "_q1"] for k in names]
    fitted = control.maketraj_batch(q0s, q1s, [d[k + "_y"] for k in names], 2.0, solver=fitter)
    assert len(fitted) == 3 and fitted.points.shape == (3, 21, 3) and fitted.vpoints.shape == (3, 20, 3)
    assert fitted.apoints.shape == (3, 19, 3) and fitted.ok.dtype == bool and fitted.t_max == 2.0
    trajs = fitted.curves(1)
    assert np.array_equal(np.array(trajs[1].control_points_), fitted.vpoints[1])
    assert np.array_equal(np.array(trajs[2].control_points_), fitted.apoints[1])
    path = tmp_path / "trajectory.json"
    control.save_trajectory(str(path), trajs)
    back = control.load_trajectory(str(path))
    for a, b in zip(trajs, back):
        assert np.array_equal(np.array(a.control_points_), np.array(b.control_points_))
        assert (b.T_min_, b.T_max_, b.mult_T_) == (0.0, 2.0, 1.0)  # the loader's quirk: the file's mult for every curve
    assert np.array_equal(back[0](1.3), trajs[0](1.3))


def test_ctypes_structures_match_the_header(tmp_path):
    from conftest import ROOT
    exe = str(tmp_path / "abi_probe_fit")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "abi_probe_fit.c")], check=True)
    rows = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    structs = {"ikg_bezier_set": _lib.BezierSet, "ikg_fit_params": _lib.FitParams}
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


# ---------------------------------------------------------------- C-ABI
def test_fit_entry_rejects_every_limit(d):
    lib = _lib.load()
    msg = lambda: lib.ikg_last_error().decode()
    HOST = _lib.IKG_FLAG_HOST_POINTERS
    q0, q1, y = (np.ascontiguousarray(x) for x in fc.inputs(d, "n40"))
    out = np.zeros(21 * 3)
    cost, status = np.zeros(1), np.zeros(1, dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(degree=20, ridge=0.0, T=1.0, n=40, dim=3, B=1, q0=q0, y=y, off=None, points=out, prm=True, flags=HOST):
        off = np.array([0, n], dtype=np.int64) if off is None else off
        fp = _lib.FitParams(degree, ridge, T)
        return lib.ikg_bezier_fit_batch(0, p(q0), p(q1), p(y), p(off), B, dim, C.byref(fp) if prm else None, p(points),
                                        None, None, p(cost), p(status), None, flags)

    assert call(prm=False) == -1 and "params" in msg()
    assert call(degree=5) == -1 and call(degree=21) == -1 and "degree" in msg()
    assert call(dim=0) == -1 and call(dim=33) == -1 and "dim" in msg()
    assert call(T=0.0) == -1 and call(T=-1.0) == -1 and call(T=float("inf")) == -1 and "total_time" in msg()
    assert call(ridge=-1e-3) == -1 and call(ridge=float("nan")) == -1 and "ridge" in msg()
    assert call(B=-1) == -1
    assert call(points=None) == -1 and "required" in msg()
    assert call(n=1) == -1 and "points" in msg()
    long = np.zeros((257, 3))
    assert call(n=257, y=long) == -1 and "257" in msg()
    assert call(n=16) == -1 and "ridge" in msg()  # fewer than degree - 3 points without a ridge
    assert call(degree=7, n=3) == -1
    assert call(off=np.array([1, 41], dtype=np.int64)) == -1 and "offsets" in msg()
    bad = y.copy()
    bad[7, 1] = np.nan
    assert call(y=bad) == -1 and "not finite" in msg()
    badq = q0.copy()
    badq[0] = np.inf
    assert call(q0=badq) == -1 and "not finite" in msg()
    # the parameters are checked with device pointers too (flags 0), before any device call
    assert call(degree=21, flags=0) == -1 and call(ridge=-1.0, flags=0) == -1 and call(T=0.0, flags=0) == -1
    d0 = _lib.FitParams()
    lib.ikg_fit_params_default(C.byref(d0))
    assert (d0.degree, d0.ridge, d0.total_time) == (20, 0.0, 1.0)


def test_per_state_entry_rejects_bad_curves():
    from ikgrasp.model import load_nextage, load_nextage_inertia
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ikg_model_create(C.byref(_lib.model_desc(load_nextage())), C.byref(h)) == 0
    msg = lambda: lib.ikg_last_error().decode()
    HOST = _lib.IKG_FLAG_HOST_POINTERS
    buf = np.zeros(15)
    p = buf.ctypes.data
    P = np.zeros((1, 3, 15))
    mk = lambda pts=P, n=3, t_max=1.0, mult=1.0: _lib.BezierSet(None if pts is None else pts.ctypes.data, n, 0.0, t_max,
                                                               mult)
    prm, out = _lib.rollout_params(4), _lib.RolloutOut()
    roll = lambda sq=None, sv=None, B=1: lib.ikg_control_rollout_curves(
        h, 0, p, p, None, B, C.byref(sq or mk()), C.byref(sv or mk()), C.byref(prm), C.byref(out), None, HOST)
    assert roll() == -1 and "inertia" in msg()
    assert lib.ikg_model_set_inertia(h, C.byref(_lib.inertia_desc(load_nextage_inertia()))) == 0
    for bad in (mk(pts=None), mk(n=1), mk(n=65), mk(t_max=0.0), mk(mult=float("nan"))):
        assert roll(sq=bad) == -1 and "q_curves" in msg()
        assert roll(sv=bad) == -1 and "v_curves" in msg()
    nan = P.copy()
    nan[0, 2, 4] = np.inf
    assert roll(sq=mk(pts=nan)) == -1 and "not finite" in msg()
    assert roll(B=-1) == -1
    lib.ikg_model_destroy(h)


# ---------------------------------------------------------------- one curve pair per state (emulator)
def test_equal_curves_match_the_shared_rollout(nextage, rd):
    fc.check_equal_curves_match_shared(nextage, rd, ticks=8)


def test_distinct_curves_match_single_rollouts(nextage, rd):
    fc.check_distinct_curves_match_single(nextage, rd, ticks=8)


def test_fit_then_track_against_the_rollout_oracle(fitter, nextage, rd):
    fc.check_fit_then_track(fitter.bezier_fit, nextage, rd, "emulator")
