"""The fp64 short trig step (ikg_device.hpp Trig<double>::step: three in-place
shears with t = tan(d/2) and sin d from short series) through the host
emulator, against the angle-addition form it replaced (step_addition, kept in
the header for this comparison).

From the exact (sin, cos) of a starting angle, Trig<double>::kResync = 128
consecutive steps of d run with no resync -- the longest run the solve loop
takes between two exact recomputations.  The bound is not a chosen figure: it
is what the replaced form reaches on the same inputs, measured here."""
import numpy as np

import emu as host_emu

STEPS = 128  # Trig<double>::kResync
KINC = 0.025  # Trig<double>::kIncMax


def _run(fn, d, a):
    return host_emu.math(fn, d, a).reshape(-1, 4)


def _inputs():
    grid = np.concatenate([np.linspace(-KINC, KINC, 201), [0.0, -KINC, KINC, 1e-9, -1e-9, 0.0212, -0.0212]])
    starts = np.array([0.0, 0.3, 1.0, np.pi / 2 - 0.2, 2.5, -2.0, -0.7, 3.0])
    d, a = np.meshgrid(grid, starts, indexing="ij")
    return d.ravel(), a.ravel()


def _errors(o, d, a):
    end = a.astype(np.longdouble) + STEPS * d.astype(np.longdouble)
    s, c = o[:, 2].astype(np.longdouble), o[:, 3].astype(np.longdouble)
    return (float(np.abs(s - np.sin(end)).max()), float(np.abs(c - np.cos(end)).max()),
            float(np.abs(s * s + c * c - 1).max()))


def test_shear_step_within_the_replaced_forms_bound():
    d, a = _inputs()
    assert (d == 0).any() and (d == KINC).any() and (d == -KINC).any() and np.abs(d).max() <= KINC
    new, old = _run(5, d, a), _run(6, d, a)
    assert np.array_equal(new[:, :2], old[:, :2])  # the same starting pairs
    e_new, e_old = _errors(new, d, a), _errors(old, d, a)
    print(f"after {STEPS} steps, max |s - sin|, |c - cos|, |s^2 + c^2 - 1|: shears {e_new}, angle addition {e_old}")
    assert e_old[0] < 1e-13 and e_old[1] < 1e-13  # the measured bound is itself a rounding-level one
    for got, bound in zip(e_new, e_old):
        assert got <= bound


def test_zero_step_leaves_the_pair_unchanged():
    a = np.array([0.0, 0.3, 1.0, np.pi / 2 - 0.2, 2.5, -2.0, -0.7, 3.0])
    o = _run(5, np.zeros_like(a), a)
    assert np.array_equal(o[:, 2:], o[:, :2])
    assert np.array_equal(np.signbit(o[:, 2:]), np.signbit(o[:, :2]))
