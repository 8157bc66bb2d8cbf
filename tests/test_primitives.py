"""The collision narrow phase, one shape pair at a time, at contact (CPU leg).

tests/golden/primitive_cases.npz holds shape pairs whose separation g is known
by construction (oracle/primitive_cases.py): every kind pair of {sphere, box,
cylinder, mesh-box} in both orders, every feature pair, degenerate poses.  The
gap sweep (1e-1 .. 1e-9 m separated, 1e-3 .. 1e-9 m deep) is expanded here.

  * the fixture proves itself with the collision oracle's support function and
    exact membership tests only;
  * independent closed forms agree with the construction at their own accuracy;
  * pair_collides / pair_distance (csrc/ikg_collision.hpp) through the host
    emulator meet the project's gates in both dtypes:
      boolean   == (g < 0)            for |g| >= 1e-9 m (fp64), 1e-4 m (fp32);
                                      fp64 clearances of pairs with a cylinder from 1e-7 m
      distance  |d - g| <= 1e-7 m     for g >= 1e-6 m   (fp64)
                |d - g| <= 1e-4 m     for g >= 1e-3 m   (fp32)
      intersecting  d <= 1e-9 m for depth >= 1e-9 m (fp64), d <= 1e-4 m for
                    depth >= 1e-4 m (fp32)
    Rows below a margin are counted in the report, not gated.

IKG_EMU_LIB names another emulator build (helpers.emu_path): an emulator built
from the new ikg_host_emu.hip against an older ikg_collision.hpp shows what
that narrow phase gets wrong (tools/README.md, "Narrow phase at contact").
"""
import os

import numpy as np
import pytest

import emu as host_emu
from conftest import GOLDEN

from oracle import collision_oracle as co
from oracle import planner_oracle as po
from oracle import primitive_cases as pc
from primitive_gates import check_gates, placements, robot_scene, sweep, world_scene

@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "primitive_cases.npz")))


@pytest.fixture(scope="module")
def emu_pairs():
    lib = host_emu.load_or_skip()

    def run(dtype, kA, PA, dA, kB, PB, dB):
        n = len(kA)
        kA, kB = (np.ascontiguousarray(k, dtype=np.int32) for k in (kA, kB))
        PA, dA, PB, dB = (np.ascontiguousarray(x, dtype=np.float64) for x in (PA, dA, PB, dB))
        hit = np.empty(n, dtype=np.uint8)
        d, dq = np.empty(n), np.empty(n)
        rc = lib.ikg_emu_pairs(0 if dtype == "f64" else 1, n, *[x.ctypes.data for x in (kA, PA, dA, kB, PB, dB, hit, d, dq)])
        assert rc == 0
        return hit.astype(bool), d, dq

    return run


_cache = {}


def emu_sweep(fx, emu_pairs, dtype):
    if dtype not in _cache:
        idx, gap = sweep(fx)
        PA, PB = placements(fx, idx, gap)
        hit, d, dq = emu_pairs(dtype, fx["kindA"][idx], PA, fx["dimsA"][idx], fx["kindB"][idx], PB, fx["dimsB"][idx])
        _cache[dtype] = (idx, gap, hit, d, dq)
    return _cache[dtype]


# ---------------------------------------------------------------- the fixture proves itself
@pytest.mark.parametrize("prefix", ["", "rob_"])
def test_fixture_proves_itself(fx, prefix):
    n = len(fx[prefix + "kindA"])
    worst_h = worst_s = 0.0
    for i in range(n):
        f = lambda k: fx[prefix + k][i]
        ga = {"kind": int(f("kindA")), "dims": f("dimsA")}
        gb = {"kind": int(f("kindB")), "dims": f("dimsB")}
        RA, tA, RB, c, nrm, rb = f("RA"), f("tA"), f("RB"), f("c"), f("n"), f("rb")
        if f("tag") == pc.CONCENTRIC:  # the common centre lies inside both shapes
            assert np.array_equal(c, tA) and not nrm.any() and not rb.any()
            assert pc.depth(ga["kind"], ga["dims"], RA, tA, c) > 0.01 < pc.depth(gb["kind"], gb["dims"], RB, c, c)
            continue
        assert abs(np.linalg.norm(nrm) - 1) <= 1e-14 and np.abs(RB @ RB.T - np.eye(3)).max() <= 1e-14
        for g in (0.1, 1e-3, 1e-9, -1e-9, -1e-3)[1 if prefix else 0:]:
            tB = c + g * nrm - rb
            # supporting planes: h_A(n) + h_B(-n) = -g
            hA = co.support(ga, RA, tA, nrm) @ nrm
            hB = co.support(gb, RB, tB, -nrm) @ (-nrm)
            worst_h = max(worst_h, abs(hA + hB + g))
            # the two witness points lie on their surfaces
            worst_s = max(worst_s, abs(pc.depth(ga["kind"], ga["dims"], RA, tA, c)),
                          abs(pc.depth(gb["kind"], gb["dims"], RB, tB, c + g * nrm)))
            if g < 0:  # their midpoint lies inside both shapes
                mid = c + 0.5 * g * nrm
                assert pc.depth(ga["kind"], ga["dims"], RA, tA, mid) > 0, (i, g)
                assert pc.depth(gb["kind"], gb["dims"], RB, tB, mid) > 0, (i, g)
    print(f"{prefix or 'world'}: worst |h_A(n) + h_B(-n) + g| = {worst_h:.2e}, worst surface residual = {worst_s:.2e}")
    assert worst_h <= 1e-14 and worst_s <= 1e-14


def test_fixture_covers_every_kind_and_feature_pair(fx):
    seen = set(zip(fx["kindA"], fx["featA"], fx["kindB"], fx["featB"]))
    for a in pc.KINDS:
        for b in pc.KINDS:
            for fa in pc.FEATURES[a]:
                for fb in pc.FEATURES[b]:
                    assert (a, fa, b, fb) in seen
            assert (a, pc.CENTRE, b, pc.CENTRE) in seen
    assert {pc.SPIN0, pc.COAXIAL, pc.DIAGONAL, pc.CONCENTRIC} <= set(fx["tag"])
    assert (fx["dimsA"] == pc.SLAB).all(axis=1).any() and (fx["dimsB"] == pc.SLAB).all(axis=1).any()
    # what the synthetic scenes of the GPU leg rely on: the rows use the palettes
    assert np.array_equal(fx["pal_dims"][fx["ia"]], fx["dimsA"]) and np.array_equal(fx["pal_t"][fx["ia"]], fx["tA"])
    assert np.array_equal(fx["bpal_dims"][fx["ib"]], fx["dimsB"])
    # robot rows: A's world placement is the oracle FK's
    for i in (0, len(fx["rob_ia"]) - 1):
        g = int(fx["rob_ia"][i])
        geoms = [{"kind": 0, "joint": int(fx["rob_geom_joint"][g]), "R": fx["rob_geom_R"][g],
                  "t": fx["rob_geom_t"][g], "dims": fx["rob_geom_dims"][g], "target": False}]
        R, t = co.geom_poses({"geoms": geoms}, fx["rob_q"][fx["rob_iq"][i]], np.eye(3), np.zeros(3))[0]
        assert np.array_equal(R, fx["rob_RA"][i]) and np.array_equal(t, fx["rob_tA"][i])


# ---------------------------------------------------------------- independent closed forms
def _rows(fx, ka, kb):
    return np.nonzero(np.isin(fx["kindA"], ka) & np.isin(fx["kindB"], kb) & (fx["tag"] != pc.CONCENTRIC))[0]


def _geoms(fx, i, g):
    ga = {"kind": int(fx["kindA"][i]), "dims": fx["dimsA"][i]}
    gb = {"kind": int(fx["kindB"][i]), "dims": fx["dimsB"][i]}
    return ga, fx["RA"][i], fx["tA"][i], gb, fx["RB"][i], fx["c"][i] + g * fx["n"][i] - fx["rb"][i]


def test_exact_sphere_forms_agree_with_the_construction(fx):
    """sphere/sphere, sphere/box (planner oracle) and sphere/cylinder (point to
    solid cylinder): exact formulas, coordinates up to ~4 m in float64."""
    boxes = [pc.BOX, pc.MESHBOX]
    worst = 0.0
    n = 0
    for ka, kb in (([pc.SPHERE], [pc.SPHERE]), ([pc.SPHERE], boxes), (boxes, [pc.SPHERE]),
                   ([pc.SPHERE], [pc.CYLINDER]), ([pc.CYLINDER], [pc.SPHERE])):
        for i in _rows(fx, ka, kb):
            for g in (1e-1, 1e-5, 1e-9):
                ga, RA, tA, gb, RB, tB = _geoms(fx, i, g)
                if pc.CYLINDER in (ga["kind"], gb["kind"]):
                    if ga["kind"] == pc.CYLINDER:
                        d = pc.point_cylinder_distance(ga["dims"], RA, tA, tB) - gb["dims"][0]
                    else:
                        d = pc.point_cylinder_distance(gb["dims"], RB, tB, tA) - ga["dims"][0]
                else:
                    d = po.pair_distance(ga, RA, tA, gb, RB, tB)
                worst = max(worst, abs(d - g))
                n += 1
    print(f"closed forms vs construction: worst |d - g| = {worst:.2e} over {n}")
    assert n > 500 and worst <= 1e-14


def test_box_box_sat_and_least_squares_agree_with_the_construction(fx):
    boxes = [pc.BOX, pc.MESHBOX]
    rows = _rows(fx, boxes, boxes)
    assert len(rows) >= 400
    for i in rows:  # the 15-axis test decides every gap of the sweep
        for g in (1e-1, 1e-6, 1e-9, -1e-9, -1e-6, -1e-3):
            ga, RA, tA, gb, RB, tB = _geoms(fx, i, g)
            hit, _ = pc.box_box_sat(RA, tA, ga["dims"], RB, tB, gb["dims"])
            assert hit == (g < 0), (i, g)
            assert co.collide(ga, RA, tA, gb, RB, tB) == (g < 0), (i, g)
    worst = 0.0
    for i in rows[::4]:  # bounded least squares (BVLS): an active-set solve, exact up to its linear algebra
        for g in (1e-1, 1e-3, 1e-6):
            ga, RA, tA, gb, RB, tB = _geoms(fx, i, g)
            worst = max(worst, abs(po.pair_distance(ga, RA, tA, gb, RB, tB) - g))
    print(f"least-squares box/box vs construction: worst |d - g| = {worst:.2e}")
    assert worst <= 1e-12


# ---------------------------------------------------------------- the device functions (emulator)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pair_collides_at_contact(fx, emu_pairs, dtype):
    idx, gap, hit, d, _ = emu_sweep(fx, emu_pairs, dtype)
    bad = check_gates(f"primitives_emu_collides_{dtype}", fx, idx, gap, hit, None, dtype)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pair_distance_at_contact(fx, emu_pairs, dtype):
    """pair_distance<T> on T-rounded placements."""
    idx, gap, hit, d, _ = emu_sweep(fx, emu_pairs, dtype)
    bad = check_gates(f"primitives_emu_distance_{dtype}", fx, idx, gap, hit, d, dtype)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_query_distance_at_contact(fx, emu_pairs, dtype):
    """What ikg_distance_kernel evaluates: pair_distance<double> on T-rounded placements."""
    idx, gap, hit, _, dq = emu_sweep(fx, emu_pairs, dtype)
    bad = check_gates(f"primitives_emu_query_distance_{dtype}", fx, idx, gap, hit, dq, dtype)
    assert not bad, "\n".join(bad)


def test_robot_rows_through_the_emulator(fx, emu_pairs):
    """The rows of the robot-attached scene (world placements from the oracle's FK)."""
    idx, gap = sweep(fx, "rob_")
    PA, PB = placements(fx, idx, gap, "rob_")
    for dtype in ("f64", "f32"):
        hit, d, dq = emu_pairs(dtype, fx["rob_kindA"][idx], PA, fx["rob_dimsA"][idx], fx["rob_kindB"][idx], PB,
                               fx["rob_dimsB"][idx])
        bad = check_gates(f"primitives_emu_robot_{dtype}", fx, idx, gap, hit, dq, dtype, "rob_")
        assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- scene level (pair_hit, geom_world)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scene_collision_through_the_emulator(fx, dtype):
    """The synthetic scenes of the GPU leg through ikg_emu_collision: the
    bounding-sphere rejection of pair_hit lets the row's pair through (the
    diagonal vertex rows sit on its threshold) and drops the 47 others;
    geom_world composes the robot scene's placements."""
    from ikgrasp.model import load_nextage
    host_emu.load_or_skip()
    model = load_nextage()

    def collision(scene, q, tg):
        return host_emu.collision(model, scene, q, tg, 0 if dtype == "f64" else 1)

    idx, gap = sweep(fx)
    _, PB = placements(fx, idx, gap)
    hit = np.zeros(len(idx), dtype=bool)
    for b in range(len(fx["bpal_kind"])):
        m = np.nonzero(fx["ib"][idx] == b)[0]
        hit[m] = collision(world_scene(fx, b), np.zeros((len(m), 15)), PB[m])
    bad = check_gates(f"primitives_emu_scene_{dtype}", fx, idx, gap, hit, None, dtype)
    idx, gap = sweep(fx, "rob_")
    _, PB = placements(fx, idx, gap, "rob_")
    hit = collision(robot_scene(fx), fx["rob_q"][fx["rob_iq"][idx]], PB)
    bad += check_gates(f"primitives_emu_robot_scene_{dtype}", fx, idx, gap, hit, None, dtype, "rob_")
    assert not bad, "\n".join(bad)
