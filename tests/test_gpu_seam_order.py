"""The fp64 record-free pair kernel integrates and clamps its joints stage by stage (ikg_device.hpp
arm_update_staged); the host emulator keeps the joint-by-joint form (arm_update).
Batches of 1, 32 and 33 problems (a lone pair, a full wave, a full wave plus one pair) run 130
updates, across the resync at 128:

  * dt = 1: first steps beyond kIncMax, the exact sincos runs on the staged clamp's result;
  * targets half a metre above reach at the default dt: joints sit on their limits from some
    update on;
  * aligned targets with one rolled target among them: its wave runs the general loop.

A problem's outputs are the same bits alone, in the wave of 32 and in the batch of 33.  Against
the host emulator and the C oracle: equal flags and counts, q within the fp64 tolerance of
tests/test_gpu_rare_path.py (the host build does not contract products into FMAs, so the device's
bits are not the emulator's; tests/test_seam_stage_order.py compares the two forms' bits on the
host, where both are compiled alike).  Measured on MI355X: max |q - emulator| 8.4e-15 (dt = 1),
1.7e-15 and 1.0e-15; against the C oracle 1.3e-14, 2.8e-15, 1.7e-15."""
import numpy as np
import pytest

import emu as host_emu
import rare_path_cases as rc
from ikgrasp import _lib
from ikgrasp.model import load_nextage
from ikgrasp.workload import uniform_targets

pytestmark = pytest.mark.gpu

PAIR = dict(variant=_lib.IKG_VARIANT_PAIR, ppw=32)
Q_TOL = 1e-9  # tests/test_gpu_rare_path.py
FIELDS = ("q", "err", "iters", "converged")
MAX_ITERS = 130
ROLLED = 5  # the rolled target's row


def _emu_solve(tg, **kw):
    model = load_nextage()
    return host_emu.solve(model, tg, np.zeros(15), **kw) + (_lib.model_desc(model),)


@pytest.fixture(scope="module")
def cases():
    """name -> targets [33, 12], solve parameters, the emulator's and the C oracle's answers"""
    host_emu.load()
    from oracle import c_oracle
    base = uniform_targets(64, seed=3)[:33]
    above = base.copy()
    above[:, 11] += 0.5
    rolled = base.copy()
    rolled[ROLLED] = rc.roll(base[ROLLED][None], 1e-12)[0]
    out = {}
    for name, tg, kw in (("big_first_steps", base, dict(dt=1.0, max_iters=MAX_ITERS)),
                         ("out_of_reach", above, dict(max_iters=MAX_ITERS)),
                         ("one_rolled", rolled, dict(max_iters=MAX_ITERS))):
        e = _emu_solve(tg, **kw)
        out[name] = dict(tg=tg, kw=kw, emu=e, oracle=c_oracle.solve_ex(tg, np.zeros(15), c_oracle.QR_STEP, **kw))
    # the cases are what their names say (on the CPU, before any launch)
    q, conv, it, _, desc = out["big_first_steps"]["emu"]
    assert conv.any() and (it[conv] < 10).all() and (it[~conv] == MAX_ITERS).all() and (~conv).sum() >= 8
    q, conv, it, _, desc = out["out_of_reach"]["emu"]
    lo, hi = np.array(desc.lower[:15]), np.array(desc.upper[:15])
    assert not conv.any() and (((q == lo) | (q == hi)).any(axis=1)).sum() >= 24
    assert not out["one_rolled"]["emu"][1].any()
    return out


def _same(a, i, b, j, what):
    for f in FIELDS:
        assert np.array_equal(np.asarray(getattr(a, f))[i], np.asarray(getattr(b, f))[j]), (what, f)


def _gate(g, rows, ref, what):
    q, c, it = ref[0][rows], ref[1][rows], ref[2][rows]
    gq = np.asarray(g.q)
    print(f"{what}: max |q - reference| = {np.abs(gq - q).max():.3e}")
    assert np.array_equal(np.asarray(g.converged, dtype=bool), c) and np.array_equal(np.asarray(g.iters), it), what
    assert np.abs(gq - q).max() <= Q_TOL, what


@pytest.mark.parametrize("name", ["big_first_steps", "out_of_reach", "one_rolled"])
def test_batches_of_1_32_33(solver, cases, name):
    c = cases[name]
    tg, kw = c["tg"], c["kw"]
    q0 = np.zeros(15)
    g33 = solver.solve(tg, q0, **PAIR, **kw)
    g32 = solver.solve(tg[:32], q0, **PAIR, **kw)
    for n, g in ((33, g33), (32, g32)):
        rows = np.arange(n)
        _gate(g, rows, c["emu"], f"{name}, {n} problems against the host emulator")
        _gate(g, rows, c["oracle"], f"{name}, {n} problems against the C oracle")
    _same(g33, np.arange(32), g32, np.arange(32), f"{name}: the first wave of 33 against the wave of 32")
    for r in range(33):
        g1 = solver.solve(tg[r:r + 1], q0, **PAIR, **kw)
        _same(g33, r, g1, 0, f"{name}: problem {r} of 33 against alone")
    if name == "out_of_reach":  # the device's joints sit on the limits too
        desc = c["emu"][4]
        lo, hi = np.array(desc.lower[:15]), np.array(desc.upper[:15])
        gq = np.asarray(g33.q)
        assert (((gq == lo) | (gq == hi)).any(axis=1)).sum() >= 24
