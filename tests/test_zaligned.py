"""The z-aligned target form of the frame-1 pose error (ikg_device.hpp
pose_error_f1<ZT>, selected per wave in ikg_solve.hpp pair_batch_body), on the
CPU through the host emulator: the selection test itself, and that the form
gives an aligned target the bits of the general one."""
import ctypes as C

import numpy as np
import pytest

import emu as host_emu
from ikgrasp import _lib
from ikgrasp.model import load_nextage
from ikgrasp.workload import uniform_targets


def _roll(tg, a):
    """The targets' rotations times Rx(a) (a roll about the cube's own x)."""
    out = np.array(tg, dtype=np.float64).reshape(-1, 12).copy()
    c, s = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    out[:, :9] = (out[:, :9].reshape(-1, 3, 3) @ rx).reshape(-1, 9)
    return out


@pytest.fixture(scope="module")
def emu():
    lib = host_emu.load_or_skip()
    model = load_nextage()
    desc = _lib.model_desc(model)

    def aligned(targets, dtype=0):
        npt = np.float64 if dtype == 0 else np.float32
        tg = np.ascontiguousarray(targets, dtype=npt).reshape(-1, 12)
        out = np.empty((len(tg), 2), np.uint8)
        assert 0 == lib.ikg_emu_z_aligned(C.byref(desc), dtype, tg.ctypes.data, len(tg), out.ctypes.data)
        return out.astype(bool)

    def solve(targets, q0, dtype=0, general=False, **kw):
        with host_emu.forced(general=general):
            return host_emu.solve(model, targets, q0, dtype, **kw)

    return dict(aligned=aligned, solve=solve)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("yaw", [0.0, np.pi / 4])
def test_sampler_targets_are_aligned(emu, dtype, yaw):
    """Both arms of every uniform_targets row, through the model's own hook tables."""
    for seed in (0, 1, 7):
        assert emu["aligned"](uniform_targets(256, seed=seed, yaw=yaw), dtype).all()


def test_rolled_target_is_not_aligned(emu):
    tg = uniform_targets(8, seed=3, yaw=np.pi / 4)
    assert emu["aligned"](tg).all()
    assert not emu["aligned"](_roll(tg, 1e-12)).any()
    assert not emu["aligned"](_roll(tg, -1e-12)).any()
    assert not emu["aligned"](_roll(tg, 0.3)).any()
    # a pitch, and a target whose [8] is not 1
    ry = np.array([[np.cos(1e-12), 0, 1e-12], [0, 1, 0], [-1e-12, 0, np.cos(1e-12)]])
    p = tg.copy()
    p[:, :9] = (p[:, :9].reshape(-1, 3, 3) @ ry).reshape(-1, 9)
    assert not emu["aligned"](p).any()
    s = tg.copy()
    s[:, 8] = np.nextafter(1.0, 0.0)
    assert not emu["aligned"](s).any()


def test_negative_zero_counts_as_zero(emu):
    tg = uniform_targets(8, seed=4, yaw=np.pi / 4)
    tg[:, [2, 5, 6, 7]] = -0.0
    assert emu["aligned"](tg).all()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("per_row", [False, True])
def test_selected_loop_equals_general_loop(emu, dtype, per_row):
    """Aligned targets: the selected (z-aligned) loop and the general loop forced
    from the host give the same q, err, update counts and flags."""
    tg = np.concatenate([uniform_targets(6, seed=0), uniform_targets(6, seed=5, yaw=np.pi)])
    neg = tg[-2:].copy()
    neg[:, [2, 5, 6, 7]] = -0.0
    tg = np.concatenate([tg, neg])
    assert emu["aligned"](tg, dtype).all()
    q0 = np.zeros(15)
    if per_row:  # row r starts 10 (r % 7) updates along its own trajectory from 0
        q0 = np.stack([emu["solve"](tg[r], q0, 0, max_iters=10 * (r % 7))[0][0] for r in range(len(tg))])
    a = emu["solve"](tg, q0, dtype)
    b = emu["solve"](tg, q0, dtype, general=True)
    assert a[1].any() and (~a[1]).any()  # passing and never-passing problems
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
