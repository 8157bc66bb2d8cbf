"""The collision narrow phase, one shape pair at a time, at contact (GPU leg).

The constructed pairs of tests/golden/primitive_cases.npz (see
tests/test_primitives.py for the fixture and the gates) through the public
queries, on synthetic scenes: a palette of 48 world-fixed shapes on a 2 m grid,
each paired with the scene's single target geometry, which every query row
places by its `targets` entry.  All other pairs fall to the bounding spheres,
so `collision()` is one pair's answer with the pair loop and the broad phase
in its path; `distance(.., [k])` and `target_env(.., [i])` name the pair.  One
more scene hangs the A shapes on Nextage joints (geom_world's composition)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from primitive_gates import check_gates, placements, robot_scene, sweep, world_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "primitive_cases.npz")))


@pytest.fixture(scope="module")
def solver():
    from ikgrasp.solver import IKSolver
    s = IKSolver(device=0)
    yield s
    s.close()


def _by_pair(ia, fn):
    """fn(rows of one A geometry, its index = its pair's index) scattered back."""
    out = None
    for k in np.unique(ia):
        m = np.nonzero(ia == k)[0]
        r = fn(m, int(k))
        if out is None:
            out = np.empty(len(ia), dtype=r.dtype)
        out[m] = r
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_world_scenes_at_contact(fx, solver, dtype):
    idx, gap = sweep(fx)
    _, PB = placements(fx, idx, gap)
    ia, ib = fx["ia"][idx], fx["ib"][idx]
    n = len(idx)
    assert n > 15000
    hit, env, d = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n)
    q0 = np.zeros(solver.nq)
    for b in range(len(fx["bpal_kind"])):
        m = np.nonzero(ib == b)[0]
        assert len(m)
        solver.set_collision(world_scene(fx, b))
        tg = PB[m]
        hit[m] = solver.collision(np.broadcast_to(q0, (len(m), solver.nq)), tg, dtype=dtype)
        env[m] = _by_pair(ia[m], lambda r, k: solver.target_env(tg[r], [k], dtype=dtype))
        d[m] = _by_pair(ia[m], lambda r, k: solver.distance(np.broadcast_to(q0, (len(r), solver.nq)), tg[r], [k],
                                                            dtype=dtype).astype(np.float64))
    bad = check_gates(f"primitives_gpu_collision_{dtype}", fx, idx, gap, hit, d, dtype)
    bad += check_gates(f"primitives_gpu_target_env_{dtype}", fx, idx, gap, env, d, dtype)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_robot_scene_at_contact(fx, solver, dtype):
    idx, gap = sweep(fx, "rob_")
    _, PB = placements(fx, idx, gap, "rob_")
    ia = fx["rob_ia"][idx]
    q = fx["rob_q"][fx["rob_iq"][idx]]
    solver.set_collision(robot_scene(fx))
    hit = solver.collision(q, PB, dtype=dtype)
    d = _by_pair(ia, lambda r, k: solver.distance(q[r], PB[r], [k], dtype=dtype).astype(np.float64))
    bad = check_gates(f"primitives_gpu_robot_{dtype}", fx, idx, gap, hit, d, dtype, "rob_")
    assert not bad, "\n".join(bad)
