"""The fp64 pair loop's SE(3) log keeps its small-angle forms and the near-pi axis behind one
wave-uniform rare branch (ikg_device.hpp log6_iter<COLD>); a wave none of whose
lanes is in either band runs the mid-band forms alone.  On the CPU through the host emulator:
ikg_emu_force_small_angle(1) takes the branch on every update, as a lane does whose wave-mates
hold it taken, and every output must be the bits of the run that takes it only where the
problem's own angle asks for it.  Counts against the C oracle, q within tests/test_host_emu.py's
fp64 tolerance."""
import numpy as np
import pytest

import emu as host_emu
import rare_path_cases as rc
from ikgrasp.model import load_nextage
from ikgrasp.workload import uniform_targets

Q_TOL = 1e-9  # tests/test_host_emu.py


@pytest.fixture(scope="module")
def emu():
    host_emu.load()
    model = load_nextage()

    def solve(targets, q0, general=False, small=False, **kw):
        with host_emu.forced(general=general, small_angle=small):
            return host_emu.solve(model, targets, q0, **kw)

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
