"""The one binding of the host emulator (libikgrasp_emu.so, built from
csrc/ikg_host_emu.hip): the CPU stand-in for the kernels' arithmetic that the
non-GPU suite, three GPU tests and tools/singular_probe.py judge the kernels by.

The library has no header; PROTOTYPES below is its declaration on the Python
side, one row per `extern "C"` export, and tests/test_emu_binding.py holds it
against the C definitions.  A new export needs a row here.

`load()` / `load_or_skip()` return the prototyped handle; a call that only one
file makes stays in that file and goes through it.  The numpy-in / numpy-out
wrappers further down are the calls several files used to restate."""
import contextlib
import ctypes as C
import os

import numpy as np

import helpers
from ikgrasp import _lib

vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double

# name -> (restype, [argtypes]); descriptor and parameter structs are c_void_p (callers pass C.byref)
PROTOTYPES = {
    "ikg_emu_big_count": (C.c_longlong, [i32]),
    "ikg_emu_lq_count": (C.c_longlong, [i32]),
    "ikg_emu_jacobi_count": (C.c_longlong, [i32]),
    "ikg_emu_svd_count": (C.c_longlong, [i32]),
    # d, dtype, targets, q0, q0_stride, B, p, q_out, conv, iters, err, trace, trace_len, cd
    "ikg_emu_solve": (i32, [vp, i32, vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, vp]),
    "ikg_emu_force_general": (None, [i32]),
    "ikg_emu_force_small_angle": (None, [i32]),
    # d, staged, n, arm, dt, in, cs_in, out
    "ikg_emu_seam": (i32, [vp, i32, i64, vp, f64, vp, vp, vp]),
    # d, dtype, targets, n, out
    "ikg_emu_z_aligned": (i32, [vp, i32, vp, i64, vp]),
    "ikg_emu_model_info": (i32, [vp, vp]),
    # d, cd, dtype, q, targets, B, out
    "ikg_emu_collision": (i32, [vp, vp, i32, vp, vp, i64, vp]),
    # d, cd, dtype, pair, qc, target, q, B, r_out, covered
    "ikg_emu_ball_cert": (i32, [vp, vp, i32, i32, vp, vp, vp, i64, vp, vp]),
    # kindA, RA, tA, dA, kindB, RB, tB, dB, r, depth
    "ikg_emu_epa": (i32, [i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
    # dtype, n, kindA, PA, dA, kindB, PB, dB, hit, dist, dist_query
    "ikg_emu_pairs": (i32, [i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    # fn, n, x, y, out
    "ikg_emu_math": (i32, [i32, i64, vp, vp, vp]),
    # fn, n, M, prev, out
    "ikg_emu_se3": (i32, [i32, i64, vp, vp, vp]),
    # d, id, dtype, q, v, B, M, nle, g
    "ikg_emu_dynamics": (i32, [vp, vp, i32, vp, vp, i64, vp, vp, vp]),
    # d, id, q, v, J, dJv, err, derr, B, p, tau, qdd, xdd, Lambda, fc
    "ikg_emu_control_torque": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
    # d, q, v, qd, vd, B, J, dJv, err, derr
    "ikg_emu_frame_terms": (i32, [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]),
    # d, id, q, v, tau, B, qdd
    "ikg_emu_forward_dynamics": (i32, [vp, vp, vp, vp, vp, i64, vp]),
    # points, n_points, dim, t_min, t_max, mult, times, K, out
    "ikg_emu_bezier": (i32, [vp, i32, i32, f64, f64, f64, vp, i64, vp]),
    # d, id, q0, v0, t0, B, bq, bv, p, out
    "ikg_emu_control_rollout": (i32, [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]),
    # d, id, q0, v0, t0, B, sq, sv, p, out
    "ikg_emu_control_rollout_curves": (i32, [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]),
    # q0, q1, y, offsets, B, dim, prm, points, vpoints, apoints, cost, status
    "ikg_emu_bezier_fit": (i32, [vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp]),
    # A, B, alpha, C, out
    "ikg_emu_se3_interpolate": (i32, [vp, vp, vp, i64, vp]),
    # nodes, cap, counts, queries, nq, P, index, dist
    "ikg_emu_nearest": (i32, [vp, i64, vp, vp, i32, i64, vp, vp]),
    # d, cd, q_curr, cube_curr, cube_rand, C, step_size, max_nodes, geoms, n_geoms, p, robot_path, cube_path,
    # n_nodes, status, steps_run
    "ikg_emu_project_paths": (i32, [vp, vp, vp, vp, vp, i64, f64, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
    # d, cd, curves, B, cube_fixed, pair_idx, n_pairs, p, out
    "ikg_emu_trajectory_check": (i32, [vp, vp, vp, i64, vp, vp, i32, vp, vp]),
    # d, id, curves, B, p, out
    "ikg_emu_trajectory_dynamics": (i32, [vp, vp, vp, i64, vp, vp]),
}

_loaded = {}  # path -> prototyped handle


def load():
    """The emulator named by helpers.emu_path() (IKG_EMU_LIB, else the in-tree
    build), opened once per path, every export under its PROTOTYPES row."""
    path = helpers.emu_path()
    if path not in _loaded:
        if not os.path.exists(path):
            raise RuntimeError(f"libikgrasp_emu.so not built (make -C <pkg>/csrc emu): {path}")
        lib = C.CDLL(path)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _loaded[path] = lib
    return _loaded[path]


def load_or_skip():
    """load(), for the suites that skip without the library."""
    import pytest
    if not os.path.exists(helpers.emu_path()):
        pytest.skip("libikgrasp_emu.so not built")
    return load()


def _ptr(a):
    return None if a is None else a.ctypes.data


def solve(model, targets, q0, dtype=0, scene=None, trace=None, **params):
    """ikg_emu_solve -> (q, converged, iters, err).  A 1-D q0 is shared by every
    problem (stride 0: the kernels' broadcast-q0 trig rule), a 2-D q0 holds a row
    per problem (stride nq); scene: the collision term; trace [B, L, 2] of the
    solve's dtype receives both hands' error norms of the first L updates;
    params: ikg_params fields."""
    npt = np.float64 if dtype == 0 else np.float32
    tg = np.ascontiguousarray(targets, dtype=npt).reshape(-1, 12)
    B, nq = len(tg), model.nq
    q0 = np.ascontiguousarray(q0, dtype=npt)
    desc = _lib.model_desc(model)
    cd = _lib.collision_desc(scene) if scene is not None else None
    params.setdefault("check_collision", int(scene is not None))
    p = _lib.default_params(**params)
    if trace is not None:
        assert trace.dtype == npt and trace.flags.c_contiguous and trace.shape == (B, trace.shape[1], 2)
    q, conv, it, err = np.empty((B, nq), npt), np.empty(B, np.uint8), np.empty(B, np.int32), np.empty((B, 2), npt)
    assert load().ikg_emu_solve(C.byref(desc), int(dtype), tg.ctypes.data, q0.ctypes.data, 0 if q0.ndim == 1 else nq, B,
                                C.byref(p), q.ctypes.data, conv.ctypes.data, it.ctypes.data, err.ctypes.data,
                                _ptr(trace), 0 if trace is None else trace.shape[1],
                                C.byref(cd) if cd is not None else None) == 0
    return q, conv.astype(bool), it, err


def counter(name, reset=True):
    """ikg_emu_<name>_count (big, lq, jacobi, svd) of this thread since its last reset."""
    return int(getattr(load(), f"ikg_emu_{name}_count")(int(reset)))


@contextlib.contextmanager
def forced(general=False, small_angle=False):
    """Run the body with the emulator's loop switches set: the general pose error
    for z-aligned targets too, log6's rare branch on every update.  Both are
    off again afterwards."""
    lib = load()
    lib.ikg_emu_force_general(int(general))
    lib.ikg_emu_force_small_angle(int(small_angle))
    try:
        yield
    finally:
        lib.ikg_emu_force_general(0)
        lib.ikg_emu_force_small_angle(0)


def math(fn, x, y=None):
    """ikg_emu_math: the loop's own math function `fn` on x (and y; x where None) -> flat,
    4 values per input for the trig steps (fn 5, 6), else room for 2 (sin, cos; atan2 fills 1)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    out = np.empty((4 if fn in (5, 6) else 2) * len(x), dtype=np.float64)
    assert load().ikg_emu_math(int(fn), len(x), x.ctypes.data, y.ctypes.data, out.ctypes.data) == 0
    return out


def collision(model, scene, q, targets, dtype=0):
    """ikg_emu_collision: the device narrow phase of `scene` at q [B,nq], targets [B,12] -> bool [B]."""
    npt = np.float64 if dtype == 0 else np.float32
    q = np.ascontiguousarray(q, dtype=npt).reshape(-1, model.nq)
    tg = np.ascontiguousarray(targets, dtype=npt).reshape(-1, 12)
    assert len(q) == len(tg)
    md, cd = _lib.model_desc(model), _lib.collision_desc(scene)
    out = np.empty(len(q), np.uint8)
    assert load().ikg_emu_collision(C.byref(md), C.byref(cd), int(dtype), q.ctypes.data, tg.ctypes.data, len(q),
                                    out.ctypes.data) == 0
    return out.astype(bool)


def se3_interpolate(A, B, alpha):
    """ikg_emu_se3_interpolate: A, B [C,12], alpha [C] -> [C,12]."""
    A, B, alpha = (np.ascontiguousarray(x, dtype=np.float64) for x in (A, B, alpha))
    out = np.empty_like(A)
    assert load().ikg_emu_se3_interpolate(A.ctypes.data, B.ctypes.data, alpha.ctypes.data, len(A), out.ctypes.data) == 0
    return out


def dynamics(model, inertias, q, v=None, dtype=0, outputs=("M", "nle", "g")):
    """ikg_emu_dynamics at q, v [B,nq] -> {name: array} of `outputs`."""
    npt = np.float64 if dtype == 0 else np.float32
    nq = model.nq
    q = np.ascontiguousarray(q, dtype=npt).reshape(-1, nq)
    v = None if v is None else np.ascontiguousarray(v, dtype=npt).reshape(-1, nq)
    d, idd = _lib.model_desc(model), _lib.inertia_desc(inertias)
    res = {k: np.empty((len(q), nq, nq) if k == "M" else (len(q), nq), npt) for k in outputs}
    assert load().ikg_emu_dynamics(C.byref(d), C.byref(idd), int(dtype), q.ctypes.data, _ptr(v), len(q),
                                   *[_ptr(res.get(k)) for k in ("M", "nle", "g")]) == 0
    return res


CONTROL_IN = ("q", "v", "J", "dJv", "err", "derr")
CONTROL_OUT = ("tau", "qdd", "xdd", "Lambda", "fc")


def control_torque(model, inertias, q, v, J, dJv, err, derr, outputs=CONTROL_OUT, **gains):
    """ikg_emu_control_torque (fp64) on B states and their kinematic terms -> {name: array} of `outputs`."""
    ins = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (q, v, J, dJv, err, derr)]
    B, nq = len(ins[0]), model.nq
    d, idd, prm = _lib.model_desc(model), _lib.inertia_desc(inertias), _lib.control_params(**gains)
    shape = {"tau": (B, nq), "qdd": (B, nq), "xdd": (B, 12), "Lambda": (B, 2, 36), "fc": (B, 12)}
    res = {k: np.empty(shape[k]) for k in outputs}
    assert load().ikg_emu_control_torque(C.byref(d), C.byref(idd), *[_ptr(a) for a in ins], B, C.byref(prm),
                                         *[_ptr(res.get(k)) for k in CONTROL_OUT]) == 0
    return res
