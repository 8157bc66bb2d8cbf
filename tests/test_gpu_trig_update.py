"""The fp64 update loop with the in-place trig step (ikg_device.hpp
Trig<double>::step: the record-free loop, the checkpoint-writing loop and the
resume loop all take it), on small batches against the C oracle:

  * the pair kernel at B = 33 (one full wave and one wave with a single
    problem), yaw 0 and yaw pi/4, with the gates of tests/test_gpu_parity.py;
  * the collision term at B = 64 with the gates of tests/test_gpu_collision.py;
  * the checkpoint loop's resync rule (ikg_solve.hpp kRsRec) is the problem's
    alone: the same 64 problems in one launch and as two launches of 32 in a
    permuted order give the same bits, and the fully regenerated records
    (IKG_BOX_COVER=0) agree as test_window_boxes_agree_with_full_regeneration
    requires.

The seeds were chosen on the CPU (oracle only) so that each batch holds every
kind of problem the loops treat differently; the tests assert that."""
import json

import numpy as np
import pytest

import helpers
from oracle import c_oracle

pytestmark = pytest.mark.gpu

SEED = 1


@pytest.fixture(scope="module")
def csolver():
    from ikgrasp.collision import load_nextage_scene
    from ikgrasp.solver import IKSolver
    s = IKSolver(device=0, scene=load_nextage_scene())
    yield s
    s.close()


@pytest.fixture(scope="module")
def col_ref():
    """The 64 targets, the oracle's loop without and with the collision term."""
    from ikgrasp.collision import load_nextage_scene
    from ikgrasp.workload import uniform_targets
    from oracle import collision_oracle
    tg = uniform_targets(64, seed=SEED)
    sc = collision_oracle.prepare(json.loads(load_nextage_scene().to_json()))
    plain = c_oracle.solve(tg, np.zeros(15))
    col = c_oracle.solve_collision(sc, tg, np.zeros(15))
    return tg, plain, col


@pytest.fixture(scope="module")
def col_one_launch(csolver, col_ref):
    return csolver.solve(col_ref[0], np.zeros(15), check_collision=True)


def _kat_rows(kat):
    return np.stack([np.concatenate([np.array(kat[k]["R"], dtype=np.float64).reshape(9),
                                     np.array(kat[k]["t"], dtype=np.float64)])
                     for k in ("cube_placement", "cube_placement_target")])


@pytest.mark.parametrize("yaw", [0.0, np.pi / 4])
def test_pair_kernel_b33_against_oracle(solver, kat, yaw):
    from ikgrasp import _lib
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(33, seed=SEED, yaw=yaw)
    q, conv, iters, err = c_oracle.solve(tg, np.zeros(15))
    assert 0 < conv.sum() < 33  # converged and unconverged problems in the batch
    sol = solver.solve(tg, np.zeros(15), dtype="f64", variant=_lib.IKG_VARIANT_PAIR)
    assert np.array_equal(sol.converged, conv)
    assert np.array_equal(sol.iters, iters)
    assert np.abs(sol.q[conv] - q[conv]).max() <= 1e-9
    assert np.abs(sol.err[conv] - err[conv]).max() <= 1e-10
    # unconverged: the iterate after max_iters agrees in end-effector space
    hg, ho = solver.fk(sol.q[~conv]), solver.fk(q[~conv])
    for h in range(2):
        e = helpers.se3_err(ho[:, h, :9].reshape(-1, 3, 3), ho[:, h, 9:], hg[:, h, :9].reshape(-1, 3, 3), hg[:, h, 9:])
        assert e.max() <= 1e-6
    k = solver.solve(_kat_rows(kat), np.zeros(15), dtype="f64", variant=_lib.IKG_VARIANT_PAIR)
    assert k.converged.all()
    assert np.abs(k.q[0] - np.array(kat["q0"])).max() <= 1e-12
    assert np.abs(k.q[1] - np.array(kat["qe"])).max() <= 1e-12


def test_collision_term_b64_against_oracle(csolver, col_ref, col_one_launch):
    tg, (_, conv0, _, _), (q, ok, iters, err) = col_ref
    cont = conv0 & ~ok  # converged but colliding at the first passing iterate: ran on
    assert ok.sum() >= 1 and cont.sum() >= 1 and (~conv0).sum() >= 1
    sol = col_one_launch
    assert np.array_equal(sol.converged, ok)
    assert np.array_equal(sol.iters, iters)
    assert np.abs(sol.q[ok] - q[ok]).max() <= 1e-9
    assert np.abs(sol.err[ok] - err[ok]).max() <= 1e-10
    assert (sol.iters[cont] == 1000).all()
    assert np.abs(sol.err[cont] - err[cont]).max() <= 1e-9
    assert csolver.collision(sol.q[cont], tg[cont]).all()


def test_window_rule_is_per_problem(csolver, col_ref, col_one_launch, monkeypatch):
    tg = col_ref[0]
    a = col_one_launch
    perm = np.random.default_rng(SEED).permutation(64)
    assert not np.array_equal(perm, np.arange(64))
    for half in (perm[:32], perm[32:]):
        b = csolver.solve(tg[half], np.zeros(15), check_collision=True)
        assert np.array_equal(b.q, a.q[half]) and np.array_equal(b.err, a.err[half])
        assert np.array_equal(b.converged, a.converged[half]) and np.array_equal(b.iters, a.iters[half])
    monkeypatch.setenv("IKG_BOX_COVER", "0")  # every colliding problem's records regenerated
    c = csolver.solve(tg, np.zeros(15), check_collision=True)
    assert np.array_equal(a.converged, c.converged) and np.array_equal(a.iters, c.iters)
    assert np.abs(a.q - c.q).max() <= 1e-12 and np.abs(a.err - c.err).max() <= 1e-12
