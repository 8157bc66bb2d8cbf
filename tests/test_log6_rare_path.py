"""The fp64 pair loop's SE(3) log keeps its small-angle forms and the near-pi axis behind one
wave-uniform rare branch (ikg_device.hpp log6_iter<COLD>); a wave none of whose
lanes is in either band runs the mid-band forms alone.  On the CPU through the host emulator:
ikg_emu_force_small_angle(1) takes the branch on every update, as a lane does whose wave-mates
hold it taken, and every output must be the bits of the run that takes it only where the
problem's own angle asks for it.  Counts against the C oracle, q within tests/test_host_emu.py's
fp64 tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import rare_path_cases as rc
from ikgrasp import _lib
from ikgrasp.model import load_nextage
from ikgrasp.workload import uniform_targets

EMU = helpers.emu_path()
Q_TOL = 1e-9  # tests/test_host_emu.py


@pytest.fixture(scope="module")
def emu():
    assert os.path.exists(EMU), "libikgrasp_emu.so not built (make -C csrc emu)"
    lib = C.CDLL(EMU)
    vp = C.c_void_p
    lib.ikg_emu_solve.argtypes = [vp, C.c_int, vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int, vp]
    for f in (lib.ikg_emu_force_general, lib.ikg_emu_force_small_angle):
        f.argtypes = [C.c_int]
        f.restype = None
    desc = _lib.model_desc(load_nextage())

    def solve(targets, q0, general=False, small=False, **kw):
        tg = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 12)
        B = len(tg)
        q0 = np.ascontiguousarray(q0, dtype=np.float64)
        stride = 0 if q0.ndim == 1 else 15
        p = _lib.default_params(**kw)
        q = np.empty((B, 15))
        conv = np.empty(B, np.uint8)
        it = np.empty(B, np.int32)
        err = np.empty((B, 2))
        lib.ikg_emu_force_general(1 if general else 0)
        lib.ikg_emu_force_small_angle(1 if small else 0)
        try:
            assert 0 == lib.ikg_emu_solve(C.byref(desc), 0, tg.ctypes.data, q0.ctypes.data, stride, B, C.byref(p),
                                          q.ctypes.data, conv.ctypes.data, it.ctypes.data, err.ctypes.data, None, 0,
                                          None)
        finally:
            lib.ikg_emu_force_general(0)
            lib.ikg_emu_force_small_angle(0)
        return q, conv.astype(bool), it, err

    return solve


@pytest.fixture(scope="module")
def cases():
    pool = uniform_targets(128, seed=0)
    q0 = np.zeros(15)
    cross, never = rc.pick(pool, q0, 8, 8)
    tg = np.concatenate([pool[cross], pool[never]])
    o = rc.oracle(tg, q0)
    assert o[1][:8].all() and not o[1][8:].any()
    # warm starts: the oracle's solution, and its iterate 5 updates before it passes
    warm = np.concatenate([o[0][:8], np.stack([rc.oracle(tg[r][None], q0, max_iters=int(o[2][r]) - 5)[0][0]
                                               for r in range(8)])])
    wtg = np.concatenate([tg[:8], tg[:8]])
    return dict(tg=tg, o=o, warm=warm, wtg=wtg, wo=rc.oracle(wtg, warm))


def _bits(a, b, what):
    for x, y, f in zip(a, b, ("q", "converged", "iters", "err")):
        assert np.array_equal(x, y), (what, f)


def _gate(a, o, what):
    q, c, it, _ = o
    assert np.array_equal(a[1], c) and np.array_equal(a[2], it), what
    assert np.abs(a[0][c] - q[c]).max() <= Q_TOL, what


@pytest.mark.parametrize("general", [False, True])
def test_crossing_and_never_crossing_problems(emu, cases, general):
    """eps = 1e-6, dt = 0.05, broadcast q0: 8 problems pass after their angles cross kPrec3,
    8 never cross."""
    a = emu(cases["tg"], np.zeros(15), general=general, **rc.PARAMS)
    b = emu(cases["tg"], np.zeros(15), general=general, small=True, **rc.PARAMS)
    _bits(a, b, "forced against own")
    assert a[1][:8].all() and not a[1][8:].any()
    _gate(a, cases["o"], "against the C oracle")


@pytest.mark.parametrize("general", [False, True])
def test_warm_starts_below_the_threshold(emu, cases, general):
    """A q0 row per problem (the medium-range trig rule): the oracle's solution and its iterate
    five updates earlier, the angle below kPrec3 from update 0."""
    a = emu(cases["wtg"], cases["warm"], general=general, **rc.PARAMS)
    b = emu(cases["wtg"], cases["warm"], general=general, small=True, **rc.PARAMS)
    _bits(a, b, "warm starts")
    _gate(a, cases["wo"], "warm starts against the C oracle")
    assert (a[2][:8] == 0).all()  # started at the solution: passes at update 0


def test_started_at_its_solution(emu, cases):
    p = dict(rc.PARAMS, max_iters=50)
    a = emu(cases["tg"][:1], cases["o"][0][0], **p)
    b = emu(cases["tg"][:1], cases["o"][0][0], small=True, **p)
    _bits(a, b, "one problem at its solution")
    assert a[1][0] and a[2][0] == 0


@pytest.mark.parametrize("general", [False, True])
def test_benchmark_targets_at_default_parameters(emu, general):
    tg = uniform_targets(4096, seed=0)[:64]
    a = emu(tg, np.zeros(15), general=general)
    b = emu(tg, np.zeros(15), general=general, small=True)
    _bits(a, b, "64 benchmark targets")
    _gate(a, c_oracle_default(tg), "benchmark targets against the C oracle")


def c_oracle_default(tg):
    from oracle import c_oracle
    return c_oracle.solve_ex(tg, np.zeros(15), c_oracle.QR_STEP)
