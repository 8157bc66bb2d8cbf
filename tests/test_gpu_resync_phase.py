"""The pair loop around its resync updates (ikg_solve.hpp, the record-free frame-1 loop): the
carried trig and the tracked rotation angle are recomputed exactly every Trig<T>::kResync updates
(fp64: 128, fp32: 16), the phase is a mask of the update count, and the tracked increment runs
on every update and is discarded on a resync one.  The loop is made to end just before, on and
just after a resync update and to run through two of them, and pairs are made to pass on one.

Launches as in tests/test_gpu_loop_exit.py, whose gates these are: pair layout, 32 problems per
wave, the first 33 of bench.py's targets (the second wave holds one live pair), against the C
oracle with the QR step.  fp64: flags and update counts equal, q within 1e-9 and err within
1e-10.  Nothing converges from q0 = 0 within 257 updates, so there q and err are compared on every
problem, as test_short_loops_fp64 does.  fp32: that file's fp32 gates (flags equal, counts within
+-2 on converged problems, end effectors within 1e-4) and a problem's outputs bit for bit those of
the same problem solved alone; where nothing has converged yet the end effectors of every problem
are held to the same 1e-4 (at most 33 updates of fp32 rounding, against the ~740 of an answer).
"""
import numpy as np
import pytest

import helpers
from test_gpu_loop_exit import EE_TOL, ERR_TOL, PAIR, Q_TOL, _alone32, _gates32, _gates64, _oracle

pytestmark = pytest.mark.gpu

RESYNC64, RESYNC32 = 128, 16  # Trig<double>::kResync, Trig<float>::kResync (ikg_device.hpp)


@pytest.fixture(scope="module")
def cases():
    """Targets, and per-row starts part-way along a problem's own trajectory: computed once."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(64, seed=0)[:33]
    q0 = np.zeros(15)
    _, c, it, _ = _oracle(tg, q0)
    conv = np.nonzero(c)[0]
    assert len(conv) >= 2 and it[conv].min() > 2 * RESYNC64

    def rows(left):
        """(problem, updates left to its passing count) -> targets, q0 rows and the oracle's run."""
        rtg = np.stack([tg[p] for p, _ in left])
        rq0 = np.stack([_oracle(tg[p][None], q0, max_iters=int(it[p]) - n)[0][0] for p, n in left])
        o = _oracle(rtg, rq0)
        assert o[1].all() and o[2].tolist() == [n for _, n in left]  # the oracle resumes its own iterates exactly
        return rtg, rq0, o

    a, b = int(conv[0]), int(conv[1])
    # fp64: pairs that pass one update before, on and after the first resync update, on the second
    # one, and well before either
    r64 = rows([(a, RESYNC64 - 1), (a, RESYNC64), (a, RESYNC64 + 1), (b, 2 * RESYNC64), (b, RESYNC64), (b, 40)])
    # fp32: the fp32 loop's passing count is the oracle's +-2, so a run of starts around the
    # resync count (two problems) puts a pair on it
    r32 = rows([(p, n) for p in (a, b) for n in range(RESYNC32 - 3, RESYNC32 + 4)] + [(a, 2 * RESYNC32)])
    return dict(tg=tg, r64=r64, r32=r32)


@pytest.mark.parametrize("max_iters", [127, 128, 129, 257])
def test_loop_ends_around_a_resync_fp64(solver, cases, max_iters):
    tg = cases["tg"]
    g = solver.solve(tg, np.zeros(15), max_iters=max_iters, **PAIR)
    o = _oracle(tg, np.zeros(15), max_iters=max_iters)
    _gates64(g, o, f"max_iters={max_iters}")
    dq, de = np.abs(g.q - o[0]).max(), np.abs(g.err - o[3]).max()
    print(f"max_iters={max_iters}: every problem, max |dq| {dq:.2e}, max |derr| {de:.2e}")
    assert dq <= Q_TOL and de <= ERR_TOL


def test_pairs_pass_on_a_resync_fp64(solver, cases):
    rtg, rq0, o = cases["r64"]
    g = solver.solve(rtg, rq0, **PAIR)
    _gates64(g, o, "per-row q0")
    assert RESYNC64 in g.iters and 2 * RESYNC64 in g.iters


def _ee_all(solver, g, q):
    ha, hb = solver.fk(g.q.astype(np.float64)), solver.fk(q)
    return max(helpers.se3_err(ha[:, h, :9].reshape(-1, 3, 3), ha[:, h, 9:], hb[:, h, :9].reshape(-1, 3, 3),
                               hb[:, h, 9:]).max() for h in range(2))


@pytest.mark.parametrize("max_iters", [15, 16, 17, 33])
def test_loop_ends_around_a_resync_fp32(solver, cases, max_iters):
    tg = cases["tg"]
    g = solver.solve(tg, np.zeros(15), dtype="f32", max_iters=max_iters, **PAIR)
    o = _oracle(tg, np.zeros(15), max_iters=max_iters)
    _gates32(solver, g, o, f"fp32 max_iters={max_iters}")
    assert np.array_equal(g.iters[~o[1]], o[2][~o[1]])  # unconverged: the loop ran to max_iters
    ee = _ee_all(solver, g, o[0])
    print(f"fp32 max_iters={max_iters}: every problem, end effectors within {ee:.2e}")
    assert ee <= EE_TOL
    _alone32(solver, tg, np.zeros(15), g, [0, 16, 32], max_iters=max_iters)


def test_pairs_pass_on_a_resync_fp32(solver, cases):
    rtg, rq0, o = cases["r32"]
    g = solver.solve(rtg, rq0, dtype="f32", **PAIR)
    _gates32(solver, g, o, "fp32 per-row q0")
    print("fp32 per-row q0: passing counts", g.iters.tolist())
    assert RESYNC32 in g.iters
    _alone32(solver, rtg, rq0, g, range(len(rtg)))
