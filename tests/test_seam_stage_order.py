"""The fp64 record-free pair loop integrates and clamps its joints stage by stage (ikg_device.hpp
arm_update_staged, DESIGN.md 3a.12: all integrates, all maxima, all minima): the same expression
trees as arm_update (the limits-in-registers path), in another order.  On the CPU through the host
emulator (ikg_emu_seam: the clamp, then the trig advance the loop runs on its result): every
output of the staged form must be the bits of the joint-by-joint form, for both arms, with and
without a resync, over

  * steps of 0, +-1e-300, +-1e-9 and +-kIncMax exactly, just inside kIncMax and just outside it
    (the exact sincos overwrites the step), in the chest, in every arm joint and in the two trig
    slots whose step is a sum of two joints' steps;
  * (s, c) at 0, pi/2, pi and random angles;
  * joints that land below, on and above either limit (dt = 1 and dt = 0.01)."""
import ctypes as C

import numpy as np
import pytest

import emu as host_emu
from ikgrasp import _lib
from ikgrasp.model import load_nextage

KINC = 0.025  # Trig<double>::kIncMax
STEPS = [0.0, 1e-300, -1e-300, 1e-9, -1e-9, KINC, -KINC, np.nextafter(KINC, 0), -np.nextafter(KINC, 0),
         KINC * (1 - 1e-9), -KINC * (1 - 1e-9), 0.0212, -0.02, np.nextafter(KINC, 1), -np.nextafter(KINC, 1), 0.1]


@pytest.fixture(scope="module")
def seam():
    lib = host_emu.load()
    desc = _lib.model_desc(load_nextage())
    lo = np.array([[desc.lower[desc.root_q]] + [desc.lower[desc.arm_q[a][k]] for k in range(6)] for a in range(2)])
    hi = np.array([[desc.upper[desc.root_q]] + [desc.upper[desc.arm_q[a][k]] for k in range(6)] for a in range(2)])

    def run(staged, arm, dt, step, q, sn, cs, resync):
        """step, q: [n][7] (chest first); sn, cs: [n][7]; arm, resync: [n]"""
        n = len(q)
        x = np.empty((n, 22))
        x[:, 0:7] = step
        x[:, 7:14] = q
        x[:, 14:21] = sn
        x[:, 21] = resync
        arm = np.ascontiguousarray(arm, dtype=np.int32)
        cs = np.ascontiguousarray(cs, dtype=np.float64)
        out = np.empty((n, 21))
        assert 0 == lib.ikg_emu_seam(C.byref(desc), staged, n, arm.ctypes.data, dt, x.ctypes.data, cs.ctypes.data,
                                     out.ctypes.data)
        return out

    return run, lo, hi


def _pairs(n, rng):
    """n rows of seven (s, c): 0, pi/2, pi in turn, then random angles"""
    a = rng.uniform(-np.pi, np.pi, (n, 7))
    a[0::4] = 0.0
    a[1::4] = np.pi / 2
    a[2::4] = np.pi
    return np.sin(a), np.cos(a)


def _check(seam, arm, dt, step, q, resync, rng):
    run = seam[0]
    sn, cs = _pairs(len(q), rng)
    a = run(0, arm, dt, step, q, sn, cs, resync)
    b = run(1, arm, dt, step, q, sn, cs, resync)
    assert np.array_equal(a, b), np.argwhere(a != b)[:8]
    assert np.array_equal(np.signbit(a), np.signbit(b))
    return a, sn, cs


def test_steps_at_the_series_edges(seam):
    """From q = 0 (inside every limit) with dt = 1 a joint's step is its dq exactly.  One joint
    moves at a time (slots 0 and 3 see its step alone), then two joints whose steps add up in
    slot 0 (chest + first arm joint) and slot 3 (third + fourth arm joint)."""
    _, lo, hi = seam
    assert (lo < -0.11).all() and (hi > 0.11).all()
    rng = np.random.default_rng(0)
    rows = []
    for d in STEPS:
        for j in range(7):
            r = np.zeros(7)
            r[j] = d
            rows.append(r)
        for j0, j1 in ((0, 1), (3, 4)):
            r = np.zeros(7)
            r[j0], r[j1] = d / 2, d / 2  # the sum is d exactly
            rows.append(r)
            r = np.zeros(7)
            r[j0], r[j1] = d, -d  # a zero slot step from two steps of size |d|
            rows.append(r)
    step = np.array(rows)
    for arm in (0, 1):
        for rs in (0.0, 1.0):
            n = len(step)
            out, sn, cs = _check(seam, np.full(n, arm), 1.0, step, np.zeros((n, 7)), np.full(n, rs), rng)
            assert np.array_equal(out[:, :7], step)  # no clamp: q + dq
            if rs == 0.0:
                still = (step == 0).all(axis=1)
                assert still.any() and np.array_equal(out[still, 7:14], sn[still]) and np.array_equal(out[still, 14:], cs[still])


def test_random_steps_and_pairs(seam):
    _, lo, hi = seam
    rng = np.random.default_rng(1)
    n = 4096
    arm = rng.integers(0, 2, n)
    q = rng.uniform(0.9 * lo[arm], 0.9 * hi[arm])
    step = rng.uniform(-0.012, 0.012, (n, 7))  # a slot's sum stays inside kIncMax
    step[::7] *= 3.0  # some rows beyond it: the exact path
    _check(seam, arm, 1.0, step, q, (rng.random(n) < 0.1).astype(float), rng)
    _check(seam, arm, 0.01, 100.0 * step, q, np.zeros(n), rng)


@pytest.mark.parametrize("dt", [1.0, 0.01])
def test_joints_at_their_limits(seam, dt):
    """Every joint in turn lands below, on and above its lower and its upper limit; the others
    move by a short step.  A clamped joint's slot step is what the clamp left of it."""
    _, lo, hi = seam
    rng = np.random.default_rng(2)
    rows_q, rows_s, rows_a = [], [], []
    for arm in (0, 1):
        for j in range(7):
            for lim, sign in ((lo[arm][j], -1.0), (hi[arm][j], 1.0)):
                for start in (lim - sign * 0.01, lim):  # 0.01 inside the limit, or on it
                    for land in (-1e-3, -1e-17, 0.0, 1e-17, 1e-3, 0.2):  # inside by / on / beyond by
                        q = rng.uniform(0.5 * lo[arm], 0.5 * hi[arm])
                        s = rng.uniform(-0.01, 0.01, 7)
                        q[j] = start
                        s[j] = (lim + sign * land) - start
                        rows_q.append(q)
                        rows_s.append(s / dt)
                        rows_a.append(arm)
    q, step, arm = np.array(rows_q), np.array(rows_s), np.array(rows_a)
    out, _, _ = _check(seam, arm, dt, step, q, np.zeros(len(q)), rng)
    assert (out[:, :7] >= lo[arm]).all() and (out[:, :7] <= hi[arm]).all()
    assert (out[:, :7] == lo[arm]).any() and (out[:, :7] == hi[arm]).any()
