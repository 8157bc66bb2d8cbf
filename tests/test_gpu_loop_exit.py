"""The pair loop's exits (ikg_solve.hpp, the record-free frame-1 loop): a pair
whose errors pass writes its outputs at that update and goes on iterating with
its wave, and the wave leaves on scalar tests (every lane's outputs written, or
the count at max_iters).  Small launches in the pair layout, 32 problems per
wave, against the C oracle (oracle/ikg_oracle.c).

fp64: the gates of tests/test_gpu_fullbatch.py::test_c2_full_fp64 -- flags and
update counts equal, q within 1e-9 and err within 1e-10 on converged problems.
The oracle runs with the same step evaluation as there (QR_STEP).

fp32: 1e-9 is below the format's resolution (an ulp of a joint angle near 1 rad
is 1.2e-7), so the fp32 cases take the fp32 gates of
test_gpu_fullbatch.py::test_c3_full_fp32 against the fp64 oracle (flags equal
or listed there as flips; here: equal, update counts within +-2 on converged
problems, end effectors within 1e-4), and what the fp32 loop can be held to
exactly: a problem's outputs are bit for bit those of the same problem solved
alone, whatever the other lanes of its wave do and however long they run.
"""
import numpy as np
import pytest

import helpers
from ikgrasp import _lib
from oracle import c_oracle

pytestmark = pytest.mark.gpu

PAIR = dict(variant=_lib.IKG_VARIANT_PAIR, ppw=32)
Q_TOL, ERR_TOL = 1e-9, 1e-10  # test_c2_full_fp64
EE_TOL = 1e-4                 # test_c3_full_fp32


@pytest.fixture(scope="module")
def cases():
    """Targets, oracle solutions from q0 = 0, and a mixed wave: computed once."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(64, seed=0)
    q0 = np.zeros(15)
    q, c, it, err = c_oracle.solve_ex(tg, q0, c_oracle.QR_STEP)
    assert c.any() and (~c).any()  # both kinds in the first 64 of bench.py's batch
    conv = np.nonzero(c)[0]
    # one wave, per-row q0: row 0 starts at an oracle solution (passes at update 0); rows
    # 1.. start part of the way along their own trajectory, so they pass at different counts;
    # the last row's target is out of reach (never passes)
    n = min(len(conv), 12)
    mtg = np.concatenate([tg[conv[:n]], tg[~c][:1]])
    mq0 = np.zeros((n + 1, 15))
    mq0[0] = q[conv[0]]
    for r in range(1, n):
        k = int(it[conv[r]]) * r // n
        mq0[r] = c_oracle.solve_ex(tg[conv[r]][None], q0, c_oracle.QR_STEP, max_iters=k)[0][0]
    far = mtg[-1].copy()
    far[9:12] += np.array([5.0, 0.0, 0.0])  # 5 m away: unreachable
    mtg[-1] = far
    mo = c_oracle.solve_ex(mtg, mq0, c_oracle.QR_STEP)
    assert mo[2][0] == 0 and mo[1][:n].all() and not mo[1][-1]
    assert len(set(mo[2][:n].tolist())) >= n // 2  # passing counts differ
    return dict(tg=tg, q=q, c=c, it=it, err=err, conv=conv, mtg=mtg, mq0=mq0, mo=mo)


def _gates64(g, o, what):
    q, c, it, err = o
    gq, gc, gi, ge = g.q, np.asarray(g.converged, dtype=bool), g.iters, g.err
    dq = np.abs(gq - q).max(axis=1)[c] if c.any() else np.zeros(1)
    de = np.abs(ge - err)[c] if c.any() else np.zeros(1)
    print(f"{what}: flags differ {int((gc != c).sum())}, counts differ {int((gi != it).sum())}, "
          f"max |dq| {dq.max():.2e}, max |derr| {de.max():.2e}")
    assert np.array_equal(gc, c), what
    assert np.array_equal(gi, it), what
    assert dq.max() <= Q_TOL and de.max() <= ERR_TOL, what


def _oracle(tg, q0, **kw):
    return c_oracle.solve_ex(tg, q0, c_oracle.QR_STEP, **kw)


@pytest.mark.parametrize("B", [1, 33, 64])
def test_batch_sizes_fp64(solver, cases, B):
    """B = 1; B = 33: the second wave holds one live pair; B = 64: two full waves."""
    g = solver.solve(cases["tg"][:B], np.zeros(15), **PAIR)
    _gates64(g, tuple(cases[k][:B] for k in ("q", "c", "it", "err")), f"B={B}")


def test_mixed_wave_fp64(solver, cases):
    """One wave: a problem that passes at update 0, problems passing at different counts, and
    an unreachable target that keeps the wave running to max_iters."""
    g = solver.solve(cases["mtg"], cases["mq0"], **PAIR)
    _gates64(g, cases["mo"], "mixed wave")
    assert g.iters[0] == 0 and np.array_equal(g.q[0], cases["mq0"][0])  # stored untouched


@pytest.mark.parametrize("max_iters", [0, 5])
def test_short_loops_fp64(solver, cases, max_iters):
    tg = cases["tg"][:33]
    g = solver.solve(tg, np.zeros(15), max_iters=max_iters, **PAIR)
    o = _oracle(tg, np.zeros(15), max_iters=max_iters)
    _gates64(g, o, f"max_iters={max_iters}")
    # nothing converges this early: q and err are compared on every problem
    assert not o[1].any()
    assert np.abs(g.q - o[0]).max() <= Q_TOL and np.abs(g.err - o[3]).max() <= ERR_TOL


def test_max_iters_at_the_passing_count_fp64(solver, cases):
    """max_iters = k0 and k0 + 1 of a problem that passes at update k0: the reference never
    tests the iterate at max_iters, so the first ends unconverged after k0 updates and the
    second converged at k0."""
    i = int(cases["conv"][0])
    k0 = int(cases["it"][i])
    tg = cases["tg"][: i + 1]
    for mi, want in ((k0, False), (k0 + 1, True)):
        g = solver.solve(tg, np.zeros(15), max_iters=mi, **PAIR)
        o = _oracle(tg, np.zeros(15), max_iters=mi)
        assert bool(o[1][i]) == want and o[2][i] == k0
        _gates64(g, o, f"max_iters={mi} (k0={k0})")
        assert np.abs(g.q[i] - o[0][i]).max() <= Q_TOL and np.abs(g.err[i] - o[3][i]).max() <= ERR_TOL


def test_whole_wave_passes_fp64(solver, cases):
    """Every problem of the wave passes, so the wave leaves before max_iters on the scalar
    exit; and the same batch as one target set with S = 4 seeds through
    solve_multistart_into, where every (target, seed) pair passes too."""
    import torch
    conv = cases["conv"][:16]
    tg = cases["tg"][conv]
    g = solver.solve(tg, np.zeros(15), **PAIR)
    o = tuple(cases[k][conv] for k in ("q", "c", "it", "err"))
    assert o[1].all() and o[2].max() < 1000
    _gates64(g, o, "whole wave passes")

    # seeds: q0 = 0 and three iterates along problem 0's own trajectory (all lead to answers)
    seeds = np.zeros((4, 15))
    for s in range(1, 4):
        seeds[s] = _oracle(tg[:1], np.zeros(15), max_iters=40 * s)[0][0]
    T, S = len(tg), len(seeds)
    per = [_oracle(tg, seeds[s]) for s in range(S)]
    assert all(p[1].all() for p in per)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    qo = torch.empty((T, 15), dtype=torch.float64, device=dev)
    cv = torch.empty(T, dtype=torch.uint8, device=dev)
    it = torch.empty(T, dtype=torch.int32, device=dev)
    er = torch.empty((T, 2), dtype=torch.float64, device=dev)
    best = torch.empty(T, dtype=torch.int32, device=dev)
    solver.solve_multistart_into(t(tg, torch.float64), t(seeds, torch.float64), qo, cv, it, er, best, _lib.IKG_F64,
                                 torch.cuda.current_stream(dev).cuda_stream, **PAIR)
    torch.cuda.synchronize()
    b = best.cpu().numpy()
    assert ((b >= 0) & (b < S)).all()
    rows = np.arange(T)
    pick = tuple(np.stack([p[k] for p in per])[b, rows] for k in range(4))
    from types import SimpleNamespace
    _gates64(SimpleNamespace(q=qo.cpu().numpy(), converged=cv.cpu().numpy().astype(bool), iters=it.cpu().numpy(),
                             err=er.cpu().numpy()), pick, "multistart S=4")
    # the winner is the seed with the smallest worse-hand error among the (all converged) seeds
    worst = np.stack([p[3].max(axis=1) for p in per])
    assert np.abs(worst[b, rows] - worst.min(axis=0)).max() <= ERR_TOL


def _gates32(solver, g, o, what):
    q, c, it, _ = o
    gc = np.asarray(g.converged, dtype=bool)
    assert np.array_equal(gc, c), what
    d = np.abs(g.iters.astype(int) - it)[c]
    ha, hb = solver.fk(g.q.astype(np.float64)), solver.fk(q)
    ee = max(helpers.se3_err(ha[:, h, :9].reshape(-1, 3, 3), ha[:, h, 9:], hb[:, h, :9].reshape(-1, 3, 3),
                             hb[:, h, 9:])[c].max() for h in range(2)) if c.any() else 0.0
    print(f"{what}: counts differ by at most {int(d.max()) if c.any() else 0}, end effectors within {ee:.2e}")
    assert (d <= 2).all() and ee <= EE_TOL, what


def _alone32(solver, tg, q0, g, rows, **kw):
    """Rows of the launch `g`, each solved in a launch of its own: the same bits."""
    for r in rows:
        a = solver.solve(tg[r][None], q0 if q0.ndim == 1 else q0[r][None], dtype="f32", **PAIR, **kw)
        assert np.array_equal(a.q[0], g.q[r]) and a.iters[0] == g.iters[r], r
        assert bool(a.converged[0]) == bool(g.converged[r]) and np.array_equal(a.err[0], g.err[r]), r


@pytest.mark.parametrize("B", [1, 33, 64])
def test_batch_sizes_fp32(solver, cases, B):
    tg = cases["tg"][:B]
    g = solver.solve(tg, np.zeros(15), dtype="f32", **PAIR)
    _gates32(solver, g, tuple(cases[k][:B] for k in ("q", "c", "it", "err")), f"fp32 B={B}")
    _alone32(solver, tg, np.zeros(15), g, sorted({0, B - 1, B // 2}))


def test_mixed_wave_fp32(solver, cases):
    g = solver.solve(cases["mtg"], cases["mq0"], dtype="f32", **PAIR)
    n = len(cases["mtg"])
    # row 0 starts at the fp64 solution rounded to fp32, which need not pass at once in fp32:
    # its flag and end effector are gated like the others', its count by the solo launch
    assert g.converged[:-1].all() and not g.converged[-1] and g.iters[-1] == 1000
    o = cases["mo"]
    _gates32(solver, g, (o[0], o[1], np.where(np.arange(n) == 0, g.iters, o[2]), o[3]), "fp32 mixed wave")
    assert len(set(g.iters[:-1].tolist())) >= (n - 1) // 2
    _alone32(solver, cases["mtg"], cases["mq0"], g, range(n))


@pytest.mark.parametrize("max_iters", [0, 5])
def test_short_loops_fp32(solver, cases, max_iters):
    tg = cases["tg"][:33]
    g = solver.solve(tg, np.zeros(15), dtype="f32", max_iters=max_iters, **PAIR)
    o = _oracle(tg, np.zeros(15), max_iters=max_iters)
    assert not g.converged.any() and (g.iters == max_iters).all()
    # a few updates from q0 = 0: fp32 rounding only (1e-5 covers 5 updates of ~1e-2 rad)
    assert np.abs(g.q - o[0]).max() <= 1e-5 and np.abs(g.err - o[3]).max() <= 1e-5
    _alone32(solver, tg, np.zeros(15), g, [0, 32], max_iters=max_iters)


def test_max_iters_at_the_passing_count_fp32(solver, cases):
    """k0 is the fp32 loop's own passing count for the problem."""
    i = int(cases["conv"][0])
    tg = cases["tg"][: i + 1]
    k0 = int(solver.solve(tg, np.zeros(15), dtype="f32", **PAIR).iters[i])
    assert abs(k0 - int(cases["it"][i])) <= 2
    a = solver.solve(tg, np.zeros(15), dtype="f32", max_iters=k0, **PAIR)
    b = solver.solve(tg, np.zeros(15), dtype="f32", max_iters=k0 + 1, **PAIR)
    assert not a.converged[i] and a.iters[i] == k0
    assert b.converged[i] and b.iters[i] == k0
    assert np.array_equal(a.q[i], b.q[i]) and np.array_equal(a.err[i], b.err[i])  # the same iterate


def test_whole_wave_passes_fp32(solver, cases):
    conv = cases["conv"][:16]
    tg = cases["tg"][conv]
    g = solver.solve(tg, np.zeros(15), dtype="f32", **PAIR)
    _gates32(solver, g, tuple(cases[k][conv] for k in ("q", "c", "it", "err")), "fp32 whole wave passes")
    assert g.converged.all() and g.iters.max() < 1000
    _alone32(solver, tg, np.zeros(15), g, [0, 15])
    seeds = np.zeros((4, 15))
    for s in range(1, 4):
        seeds[s] = _oracle(tg[:1], np.zeros(15), max_iters=40 * s)[0][0]
    m = solver.solve_multistart(tg, seeds, dtype="f32", **PAIR)
    assert m.converged.all()
    for t_ in (0, 15):  # the winner's outputs are those of that (target, seed) solved alone
        a = solver.solve(tg[t_][None], seeds[m.best_seed[t_]], dtype="f32", **PAIR)
        assert np.array_equal(a.q[0], m.q[t_]) and a.iters[0] == m.iters[t_]
