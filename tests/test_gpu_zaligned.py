"""The pair kernel's two loops (ikg_solve.hpp pair_batch_body): a wave whose
targets are all rotations about z runs the z-aligned form of the pose error
(pose_error_f1<ZT>), a wave holding any other target the general form.  The
two forms are the same expression tree with exact zeros and a one substituted,
so an aligned problem's outputs must be bit for bit the same on either loop:
solved alone, in aligned-only batches, and in a wave that also holds a rolled
target.  Against the C oracle (oracle/ikg_oracle.c): the fp64 gates of
tests/test_gpu_loop_exit.py, fp32 its fp32 gates.

Pair layout, 32 problems per wave, default max_iters: the targets are chosen
with the oracle so that passing and never-passing problems both occur.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import helpers
from ikgrasp import _lib
from oracle import c_oracle

pytestmark = pytest.mark.gpu

PAIR = dict(variant=_lib.IKG_VARIANT_PAIR, ppw=32)
Q_TOL, ERR_TOL = 1e-9, 1e-10  # tests/test_gpu_loop_exit.py
EE_TOL = 1e-4
ROLL = 1e-12
FIELDS = ("q", "err", "iters", "converged")


def _roll(tg, a):
    out = np.array(tg, dtype=np.float64).reshape(-1, 12).copy()
    c, s = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    out[:, :9] = (out[:, :9].reshape(-1, 3, 3) @ rx).reshape(-1, 9)
    return out


def _oracle(tg, q0):
    return c_oracle.solve_ex(tg, q0, c_oracle.QR_STEP)


def _pick(tg, q0, n):
    """n rows of tg, passing and never-passing ones alternating while both last (by the oracle)."""
    o = _oracle(tg, q0)
    c = o[1]
    assert c.any() and (~c).any()
    a, b = list(np.nonzero(c)[0]), list(np.nonzero(~c)[0])
    rows = []
    while len(rows) < n:
        for src in (a, b):
            if src and len(rows) < n:
                rows.append(int(src.pop(0)))
    rows = np.array(sorted(rows))
    return rows, tuple(x[rows] for x in o)


@pytest.fixture(scope="module")
def cases():
    """Per target set (identity, yawed in [-pi, pi], the yawed ones with -0.0 in the zero
    entries): 96 aligned targets with their oracle solutions from q0 = 0, and the rolled target
    with its own; computed once."""
    from ikgrasp.workload import uniform_targets
    q0 = np.zeros(15)
    out = {}
    yawed = uniform_targets(256, seed=12, yaw=np.pi)
    negz = yawed.copy()
    negz[:, [2, 5, 6, 7]] = -0.0
    for name, pool in (("identity", uniform_targets(256, seed=0)), ("yawed", yawed), ("negzero", negz)):
        rows, o = _pick(pool, q0, 96)
        tg = pool[rows]
        rolled = _roll(tg[5:6], ROLL)
        out[name] = dict(tg=tg, o=o, rolled=rolled, ro=_oracle(rolled, q0))
    # per-row q0 (the kernels' medium-range trig rule): row r starts 10 (r % 7) updates along the
    # yawed target r's own trajectory from 0, so the rows pass at different counts
    tg = out["yawed"]["tg"]
    out["q0rows"] = np.stack([c_oracle.solve_ex(tg[r][None], q0, c_oracle.QR_STEP, max_iters=10 * (r % 7))[0][0]
                              for r in range(96)])
    return out


def _same(a, i, b, j, what):
    for f in FIELDS:
        assert np.array_equal(np.asarray(getattr(a, f))[i], np.asarray(getattr(b, f))[j]), (what, f)


def _solo(solver, t, q, per_row, **kw):
    """One problem in a launch of its own.  per_row: on the kernel a per-row q0 selects (the
    medium-range trig rule, which a [1, nq] q0 does not), as two copies of the problem."""
    if per_row:
        return solver.solve(np.stack([t, t]), np.stack([q, q]), **PAIR, **kw)
    return solver.solve(t[None], q, **PAIR, **kw)


def _mixed(solver, tg, q0, rolled, rq0, pos, n, **kw):
    """A wave of n problems: tg[:n] with the rolled target put in at row pos."""
    t = tg[:n].copy()
    t[pos] = rolled
    q = q0
    if q0.ndim == 2:
        q = q0[:n].copy()
        q[pos] = rq0
    return solver.solve(t, q, **PAIR, **kw)


def _loops_agree(solver, c, q0, **kw):
    """The aligned target tg[1] (and tg[31], the last pair of the first wave): alone (the
    z-aligned loop), in aligned-only batches of 33, 64, 96, and in a wave with the rolled target
    at lane pair 0 / the middle / last (the general loop): the same bits.  The rolled target:
    the bits of its solo launch."""
    tg, rolled = c["tg"], c["rolled"][0]
    rows = q0.ndim == 2
    rq0 = q0[5] if rows else q0
    qrow = lambda r: q0[r] if rows else q0
    alone = {r: _solo(solver, tg[r], qrow(r), rows, **kw) for r in (1, 31)}
    ralone = _solo(solver, rolled, rq0, rows, **kw)
    for B in (33, 64, 96):
        g = solver.solve(tg[:B], q0[:B] if rows else q0, **PAIR, **kw)
        for r in (1, 31):
            _same(g, r, alone[r], 0, f"aligned batch B={B} row {r}")
        _same(g, B - 1, _solo(solver, tg[B - 1], qrow(B - 1), rows, **kw), 0, f"B={B} last row")
    # one wave of 32 holding the rolled target; and 33: the rolled target alone in the last wave
    for pos, n in ((0, 32), (16, 32), (31, 32), (32, 33)):
        g = _mixed(solver, tg, q0, rolled, rq0, pos, n, **kw)
        _same(g, pos, ralone, 0, f"rolled target at {pos}")
        for r in (1, 31):
            if r != pos:
                _same(g, r, alone[r], 0, f"aligned row {r} with the rolled target at {pos} of {n}")
    return alone, ralone


def _gates64(g, o, what):
    q, c, it, err = o
    gc = np.asarray(g.converged, dtype=bool)
    dq = np.abs(g.q - q).max(axis=1)[c] if c.any() else np.zeros(1)
    de = np.abs(g.err - err)[c] if c.any() else np.zeros(1)
    print(f"{what}: flags differ {int((gc != c).sum())}, counts differ {int((g.iters != it).sum())}, "
          f"max |dq| {dq.max():.2e}, max |derr| {de.max():.2e}")
    assert np.array_equal(gc, c), what
    assert np.array_equal(g.iters, it), what
    assert dq.max() <= Q_TOL and de.max() <= ERR_TOL, what


def _gates32(solver, g, o, what):
    q, c, it, _ = o
    gc = np.asarray(g.converged, dtype=bool)
    d = np.abs(g.iters.astype(int) - it)[c]
    ha, hb = solver.fk(g.q.astype(np.float64)), solver.fk(q)
    ee = max(helpers.se3_err(ha[:, h, :9].reshape(-1, 3, 3), ha[:, h, 9:], hb[:, h, :9].reshape(-1, 3, 3),
                             hb[:, h, 9:])[c].max() for h in range(2)) if c.any() else 0.0
    print(f"{what}: flags differ {int((gc != c).sum())}, counts differ by at most "
          f"{int(d.max()) if c.any() else 0}, end effectors within {ee:.2e}")
    assert np.array_equal(gc, c), what
    assert (d <= 2).all() and ee <= EE_TOL, what


@pytest.mark.parametrize("name", ["identity", "yawed", "negzero"])
def test_same_bits_on_either_loop_fp64(solver, cases, name):
    c = cases[name]
    _loops_agree(solver, c, np.zeros(15))
    # against the oracle: the aligned batch (both kinds of problem), and the rolled target in a
    # mixed wave, whose aligned rows are gated on the general loop
    g = solver.solve(c["tg"], np.zeros(15), **PAIR)
    assert g.converged.any() and not g.converged.all()
    _gates64(g, c["o"], f"{name}: 96 aligned targets")
    m = _mixed(solver, c["tg"], np.zeros(15), c["rolled"][0], None, 16, 32)
    o = tuple(np.concatenate([x[:16], y[:1], x[17:32]]) for x, y in zip(c["o"], c["ro"]))
    _gates64(m, o, f"{name}: wave with the {ROLL:g}-rolled target")


def test_same_bits_on_either_loop_fp64_per_row_q0(solver, cases):
    c, q0 = cases["yawed"], cases["q0rows"]
    _loops_agree(solver, c, q0)
    g = solver.solve(c["tg"], q0, **PAIR)
    _gates64(g, _oracle(c["tg"], q0), "per-row q0: 96 aligned targets")


@pytest.mark.parametrize("name", ["identity", "yawed", "negzero"])
def test_same_bits_on_either_loop_fp32(solver, cases, name):
    c = cases[name]
    _loops_agree(solver, c, np.zeros(15), dtype="f32")
    g = solver.solve(c["tg"], np.zeros(15), dtype="f32", **PAIR)
    _gates32(solver, g, c["o"], f"fp32 {name}: 96 aligned targets")


def test_same_bits_on_either_loop_fp32_per_row_q0(solver, cases):
    _loops_agree(solver, cases["yawed"], cases["q0rows"], dtype="f32")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_multistart_on_either_loop(solver, cases, dtype):
    """3 seeds x 8 targets (24 problems, one wave): aligned targets on the z-aligned loop, and
    the same with one target rolled (the general loop): the aligned targets' winners and their
    outputs are the same bits, and are those of that (target, seed) solved alone."""
    c = cases["yawed"]
    tg = c["tg"][:8]
    seeds = np.concatenate([np.zeros((1, 15)), cases["q0rows"][[3, 6]]])
    a = solver.solve_multistart(tg, seeds, dtype=dtype, **PAIR)
    t = tg.copy()
    t[3] = _roll(tg[3:4], ROLL)[0]
    b = solver.solve_multistart(t, seeds, dtype=dtype, **PAIR)
    keep = [i for i in range(8) if i != 3]
    assert np.array_equal(a.best_seed[keep], b.best_seed[keep])
    _same(a, keep, b, keep, "multistart, aligned against one rolled target")
    for i in (0, 7):
        s = _solo(solver, tg[i], seeds[a.best_seed[i]], True, dtype=dtype)  # multi-start: the per-row kernel
        _same(SimpleNamespace(**{f: np.asarray(getattr(a, f)) for f in FIELDS}), i, s, 0, f"winner of target {i}")
    if dtype == "f64":
        per = [_oracle(t, seeds[s]) for s in range(3)]
        pick = tuple(np.stack([p[k] for p in per])[b.best_seed, np.arange(8)] for k in range(4))
        _gates64(b, pick, "multistart with the rolled target")
