"""The fp64 record-free pair kernel takes log6_iter's rare branch (small-angle forms, near-pi
axis) per wave: when any lane's angle is in either band.  A problem's outputs must not depend on
whether its wave-mates hold the branch taken.  Problems from tests/rare_path_cases.py (eps =
1e-6, dt = 0.05: passing problems cross kPrec3 before they pass): each crossing problem alone,
in a wave of 32 crossing problems and as the one crossing problem among 31 that never cross,
bit for bit; the mirror case with warm-started mates that hold the branch taken from update 0.
Both trig-rule instantiations (broadcast q0 / a q0 row per problem) and both loops (a rolled
target sends the wave to the general loop).  Counts equal the C oracle's, q within the fp64
tolerance of tests/test_gpu_fullbatch.py."""
import numpy as np
import pytest

import rare_path_cases as rc
from ikgrasp import _lib
from ikgrasp.workload import uniform_targets

pytestmark = pytest.mark.gpu

PAIR = dict(variant=_lib.IKG_VARIANT_PAIR, ppw=32)
Q_TOL = 1e-9
FIELDS = ("q", "err", "iters", "converged")
ROLL = 1e-12


@pytest.fixture(scope="module")
def cases():
    out = {}
    q0 = np.zeros(15)
    for loop in ("zaligned", "general"):
        pool = uniform_targets(256, seed=0)
        if loop == "general":
            pool = rc.roll(pool, ROLL)
        cross, never = rc.pick(pool, q0, 32, 31)
        ct, nt = pool[cross], pool[never]
        co = rc.oracle(ct, q0)
        # warm starts of the crossing problems: the oracle's iterate two updates before passing
        warm = np.stack([rc.oracle(ct[r][None], q0, max_iters=int(co[2][r]) - 2)[0][0] for r in range(31)])
        out[loop] = dict(ct=ct, nt=nt, co=co, no=rc.oracle(nt, q0), warm=warm)
    return out


def _same(a, i, b, j, what):
    for f in FIELDS:
        assert np.array_equal(np.asarray(getattr(a, f))[i], np.asarray(getattr(b, f))[j]), (what, f)


def _gate(g, rows, o, orows, what):
    q, c, it, _ = (x[orows] for x in o)
    gc = np.asarray(g.converged, dtype=bool)[rows]
    assert np.array_equal(gc, c) and np.array_equal(np.asarray(g.iters)[rows], it), what
    if c.any():
        assert np.abs(np.asarray(g.q)[rows][c] - q[c]).max() <= Q_TOL, what


def _solve(solver, tg, per_row, q0=None):
    """per_row: a q0 row per problem selects the medium-range trig instantiation."""
    tg = np.asarray(tg).reshape(-1, 12)
    if q0 is None:
        q0 = np.zeros((len(tg), 15)) if per_row else np.zeros(15)
    if per_row and len(tg) == 1:  # a [1, nq] q0 does not select it: two copies of the problem
        return solver.solve(np.concatenate([tg, tg]), np.concatenate([q0, q0]), **PAIR, **rc.PARAMS)
    return solver.solve(tg, q0, **PAIR, **rc.PARAMS)


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("loop", ["zaligned", "general"])
def test_crossing_problem_in_three_placements(solver, cases, loop, per_row):
    """Every one of the 32 crossing problems: alone, in the wave of 32 crossing problems, and as
    the one crossing problem among 31 that never cross, at lane pair (5 r + 3) % 32 (every lane
    pair once: 5 is prime to 32)."""
    c = cases[loop]
    wave = _solve(solver, c["ct"], per_row)
    assert np.asarray(wave.converged).all()
    _gate(wave, np.arange(32), c["co"], np.arange(32), "32 crossing problems")
    # the same 32 in another lane order: a problem's bits do not depend on its lane pair either
    perm = (5 * np.arange(32) + 3) % 32
    moved = _solve(solver, c["ct"][np.argsort(perm)], per_row)
    for r in range(32):
        pos = int(perm[r])
        alone = _solve(solver, c["ct"][r], per_row)
        _same(wave, r, alone, 0, f"crossing problem {r}: wave of 32 against alone")
        _same(moved, pos, alone, 0, f"crossing problem {r}: wave of 32, lane pair {pos}")
        t = np.concatenate([c["nt"][:pos], c["ct"][r][None], c["nt"][pos:]])
        mixed = _solve(solver, t, per_row)
        _same(mixed, pos, alone, 0, f"crossing problem {r} among 31 that never cross, lane pair {pos}")
        keep = np.array([i for i in range(32) if i != pos])
        assert not np.asarray(mixed.converged)[keep].any()
        _gate(mixed, keep, c["no"], np.arange(31), "31 never-crossing problems")


@pytest.mark.parametrize("loop", ["zaligned", "general"])
def test_never_crossing_problem_among_warm_started_mates(solver, cases, loop):
    """31 mates start two updates before their solutions (the branch taken from update 0, a q0
    row per problem) and the never-crossing problem from 0: its bits are its solo launch's.
    Eight never-crossing problems, each at another lane pair."""
    c = cases[loop]
    for r in range(8):
        pos = (4 * r + (r & 1) * 3) % 32  # 0, 7, 8, 15, 16, 23, 24, 31
        alone = _solve(solver, c["nt"][r], True)
        t = np.concatenate([c["ct"][:pos], c["nt"][r][None], c["ct"][pos:31]])
        q0 = np.concatenate([c["warm"][:pos], np.zeros((1, 15)), c["warm"][pos:31]])
        g = _solve(solver, t, True, q0)
        _same(g, pos, alone, 0, f"never-crossing problem {r} among warm-started mates, lane pair {pos}")
        keep = np.array([i for i in range(32) if i != pos])
        assert np.asarray(g.converged)[keep].all() and (np.asarray(g.iters)[keep] <= 2).all()
        _gate(g, np.array([pos]), c["no"], np.array([r]), "never-crossing problem against the oracle")


def test_started_at_its_solution(solver, cases):
    c = cases["zaligned"]
    p = dict(rc.PARAMS, max_iters=50)
    g = solver.solve(c["ct"][:1], c["co"][0][0], **PAIR, **p)
    assert bool(np.asarray(g.converged)[0]) and int(np.asarray(g.iters)[0]) == 0
    assert np.abs(np.asarray(g.q)[0] - c["co"][0][0]).max() <= Q_TOL
