"""The IK loop's carried joint trig at every step size and dt, on the CPU
through the host emulator (ikg_host_emu.hip: the kernels' stage functions, one
problem at a time), against tests/golden/step_regime_cases.npz
(tests/golden/make_step_regime_golden.py).

Paths: a q0 row per problem (trig_med_f1), a broadcast q0 (the in-place short
step with the exact overwrite), the forced generic path (trig_advance<T, 2> on
joint steps), the damped step and fp32.  Every tolerance is the fixture's
bucket bound (8 A 2^-53 fp64, 8 A 2^-24 fp32 on |q - q_mp|, A = the float64
reference loop's own distance from its 32-digit evaluation; the damped path
against ik_oracle.computeqgrasppose(lam) in float64); group C keeps the
gates of tests/test_gpu_parity.py.  The GPU suite (tests/
test_gpu_step_regime.py) covers what exists on the device only: the wave-level
selection, the packed and quad layouts and the collision term's kernels."""
import os

import numpy as np
import pytest

import emu as host_emu
import helpers
import step_regime_cases as sr
from ikgrasp.model import load_nextage

GENERIC = 99  # ikg_params.variant the emulator reads as "force the generic path"
PATHS = ("rows_f64", "bcast_f64", "generic_f64", "damped_f64", "rows_f32")
Q_GATE, ERR_GATE = 1e-9, 1e-10  # tests/test_gpu_parity.py
EE_GATE = 1.4e-5  # README, C3: fp32 against the fp64 oracle's solution in end-effector space


@pytest.fixture(scope="module")
def fx():
    return sr.load()


@pytest.fixture(scope="module")
def emu():
    host_emu.load_or_skip()
    model = load_nextage()

    def solve(path, targets, q0, **kw):
        """q0 [B, 15].  A broadcast path takes each problem with its row as the one shared q0."""
        dtype = 1 if path.endswith("f32") else 0
        tg = np.reshape(targets, (-1, 12))
        q0 = np.broadcast_to(q0, (len(tg), 15))
        if path == "generic_f64":
            kw["variant"] = GENERIC
        if path == "damped_f64":
            kw["lambda_"] = sr.LAMBDA
        host_emu.counter("big")
        if path == "bcast_f64":
            q, conv, it, err = (np.concatenate(x) for x in zip(*[host_emu.solve(model, tg[i], q0[i], dtype, **kw)
                                                                 for i in range(len(tg))]))
        else:
            q, conv, it, err = host_emu.solve(model, tg, q0, dtype, **kw)
        return q.astype(np.float64), conv, it, err.astype(np.float64), host_emu.counter("big")

    return solve


_DAMPED = {}


def damped_reference(targets, q0, dt, K):
    """ik_oracle.computeqgrasppose(lam) after exactly K updates, computed once per case."""
    from oracle import ik_oracle as o
    key = (targets.tobytes(), np.asarray(q0).tobytes(), dt, K)
    if key not in _DAMPED:
        q0 = np.broadcast_to(q0, (len(targets), 15))
        _DAMPED[key] = np.array([o.computeqgrasppose(q0[i], t[:9].reshape(3, 3), t[9:], max_iters=K, dt=dt, eps=0.0,
                                                     lam=sr.LAMBDA)[0] for i, t in enumerate(targets)])
    return _DAMPED[key]


def _reference(path, fx_q_mp, targets, q0, dt, K):
    return damped_reference(targets, q0, dt, K) if path == "damped_f64" else fx_q_mp


def _bound(fx, group, path, i):
    """The bucket bound of a path."""
    return float(fx[f"{group}_bound32" if path.endswith("f32") else f"{group}_bound64"][i])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", range(len(sr.a_cases())), ids=lambda i: "{}-dt{}-K{}".format(*sr.a_cases()[i]))
def test_group_a_within_bucket_bound(emu, fx, case, path):
    lay, dt, K = sr.a_cases()[case]
    tg = fx["a_targets"]
    q0 = np.zeros((sr.N_A, 15)) if lay == "zero" else fx["a_q0_rows"]
    q, conv, it, _, big = emu(path, tg, q0, dt=dt, eps=0.0, max_iters=K)
    assert not conv.any() and (it == K).all()
    bound = _bound(fx, "a", path, case)
    d = np.abs(q - _reference(path, fx["a_q_mp"][case], tg, q0, dt, K)).max()
    print(f"{lay} dt {dt} K {K} {path}: |q - ref| = {d:.3e}, bound {bound:.3e}, ratio {d / bound:.3f}")
    assert d <= bound
    if path == "generic_f64":
        # ikg_emu_big_count: lane-updates with a joint step beyond the short range
        r = sr.a_regimes(fx, lay, dt, K, "joint", "f64")
        over, edge = int((r >= sr.MEDIUM).sum()), int((r == sr.AT_EDGE).sum())
        assert over <= big <= over + edge
        if (r == sr.EXACT).any():
            assert big > 0
        if (r == sr.SHORT).all():
            assert big == 0


@pytest.mark.parametrize("path", PATHS)
def test_group_b_on_the_thresholds(emu, fx, path):
    """The first update lands 2^-20 (relative) below or above kIncMax / kIncMed of
    either precision, in a sum slot or a plain slot: whichever rule the path
    takes there, the second update's answer meets the bucket bound."""
    worst = 0.0
    for i in range(len(fx["b_dt"])):
        tg, q0, dt = fx["b_targets"][i][None], fx["b_q0"][i][None], float(fx["b_dt"][i])
        q, _, it, _, _ = emu(path, tg, q0, dt=dt, eps=0.0, max_iters=sr.B_K)
        assert it[0] == sr.B_K
        bound = _bound(fx, "b", path, i)
        d = np.abs(q - _reference(path, fx["b_q_mp"][i][None], tg, q0, dt, sr.B_K)).max()
        worst = max(worst, d / bound)
        assert d <= bound, (i, float(fx["b_thr"][i]), int(fx["b_side"][i]), bool(fx["b_sum"][i]), d, bound)
    print(f"{path}: largest |q - ref| / bound over the 64 threshold cases {worst:.3f}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", range(2 * len(sr.C_DTS)))
def test_group_c_whole_solves(emu, fx, case, path):
    lay, dt = sr.LAYOUTS[fx["c_layout"][case]], float(fx["c_dt"][case])
    tg = fx["c_targets"]
    q0 = np.zeros((sr.N_A, 15)) if lay == "zero" else fx["c_q0_rows"]
    q, conv, it, err, _ = emu(path, tg, q0, dt=dt)
    pre = "c_damped_" if path == "damped_f64" else "c_"
    ok, ref_it, ref_q, ref_err = (fx[pre + k][case] for k in ("converged", "iters", "q", "err"))
    if path.endswith("f32"):  # README's C3 gate: equal flags, counts within one, end-effector error <= 1.4e-5
        assert np.array_equal(conv, ok) and (np.abs(it - ref_it) <= 1).all()
        model = load_nextage()
        hands = np.array([helpers.hands_from_tables(model, x) for x in q[ok]])
        hr = np.array([helpers.hands_from_tables(model, x) for x in ref_q[ok]])
        for h in range(2):
            e = helpers.se3_err(hr[:, h, :9].reshape(-1, 3, 3), hr[:, h, 9:], hands[:, h, :9].reshape(-1, 3, 3), hands[:, h, 9:])
            print(f"{lay} dt {dt} fp32 hand {h}: end-effector distance to the oracle's solution {e.max():.3e}")
            assert e.max() <= EE_GATE
        return
    assert np.array_equal(conv, ok) and np.array_equal(it, ref_it)
    assert np.abs(q[ok] - ref_q[ok]).max() <= Q_GATE
    assert np.abs(err[ok] - ref_err[ok]).max() <= ERR_GATE


def test_fixture_holds_what_the_generator_asserts(fx):
    """The coverage the other tests lean on, re-read from the committed arrays."""
    reg = fx["a_regime"]
    for pi in range(2):
        for li in range(2):
            for ki in range(2):
                r = reg[li, :, :, :, :, ki, pi]
                assert all((r == code).any() for code in (sr.SHORT, sr.MEDIUM, sr.EXACT))
    assert (fx["a_track"] == 1).any() and (fx["a_track"] == 0).any()
    assert (fx["a_bound64"] == 8 * fx["a_A"] * 2.0 ** -53).all() and (fx["a_bound32"] == 8 * fx["a_A"] * 2.0 ** -24).all()
    assert (fx["b_bound64"] == 8 * fx["b_A"] * 2.0 ** -53).all() and (fx["b_bound32"] == 8 * fx["b_A"] * 2.0 ** -24).all()
    assert np.array_equal(np.maximum(1.0, np.abs(fx["a_q_c"] - fx["a_q_mp"]).max(axis=(1, 2)) / 2.0 ** -53), fx["a_A"])
    for k in range(2):
        ok, p = fx["d_converged"][k], fx["d_converged_plain"][k]
        assert ok.any() and (p & ~ok).any() and (~p).any()
    assert os.path.getsize(sr.PATH) < 200 * 1024
