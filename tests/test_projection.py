"""Device-side path projection (ikg_project_paths) on the CPU: the fixture
tests/golden/projection_cases.npz (tests/golden/make_projection_golden.py;
shared code in tests/projection_cases.py) and the projection's bookkeeping on
the host emulator.

  * the fixture proves itself: the generator's conditions recomputed where that
    is cheap (coverage of the outcomes, step counts away from an integer or on
    it, the placement checks on the scene inflated and deflated by 1e-9, the
    recorded margins of the solves), the float64 interpolation and its recorded
    error, and the oracle's rows reproduced by planner_oracle.project_path for
    the chains with no failing solve;
  * ikg_emu_project_paths (csrc/ikg_host_emu.hip) runs the entry's host-pointer
    step loop with the kernels' own per-chain functions (project_prepare_chain,
    project_commit_chain, csrc/ikg_planner.hpp) around the emulator's collision
    solve: every chain alone, each step-size group in one call in fixture
    order, in reverse and in the GPU leg's permutation, the max_nodes edges,
    the step boundary and the host's spare step, the refusals.

Bars (projection_cases.compare): n_nodes and status equal the oracle's; q
within 1e-9 of its rows; cube rows within max(16 x the float64 restatement's
recorded error, 1e-15) of the 50-digit rows, identity rotations within 1e-15;
rows past n_nodes zero; no live status.  A chain in a batch against the same
chain alone: q within 1e-12, cube rows bitwise.
"""
import ctypes as C
import os

import numpy as np
import pytest

import emu as host_emu
import projection_cases as pj

DELTA, TIE, EPS = 1e-9, 1e-6, 1e-3


@pytest.fixture(scope="module")
def cases():
    return pj.cases()


@pytest.fixture(scope="module")
def oscenes():
    from oracle import collision_oracle as co
    out = {}
    for d in (0.0, DELTA, -DELTA):
        sc = co.load_scene(os.path.join(pj.GOLDEN, "collision_scene.json"))
        for g in sc["geoms"]:
            g["dims"] = np.maximum(g["dims"] + d * (g["dims"] > 0), 0.0)
        out[d] = sc
    return out


class Emu:
    def __init__(self):
        from ikgrasp import _lib
        from ikgrasp.collision import load_nextage_scene
        from ikgrasp.model import load_nextage
        self.lib = host_emu.load()
        scene = load_nextage_scene()
        self.md, self.cd = _lib.model_desc(load_nextage()), _lib.collision_desc(scene)
        self.env = np.ascontiguousarray(scene.env_geoms(), dtype=np.int32)
        self.target = next(k for k, g in enumerate(scene.geoms) if g.target)
        self.prm = _lib.default_params(eps=pj.SOLVE["eps"], dt=pj.SOLVE["dt"], max_iters=pj.SOLVE["max_iters"],
                                       check_collision=1)
        self.steps_run = None

    def call(self, q0, A, B, step_size, max_nodes, geoms=None, out=None):
        """-> (rc, outputs); `out`: pre-filled outputs to write into"""
        n, M = len(q0), max(int(max_nodes), 0)
        g = self.env if geoms is None else np.ascontiguousarray(geoms, dtype=np.int32)
        res = out or {"robot_path": np.empty((n, M, 15)), "cube_path": np.empty((n, M, 12)),
                      "n_nodes": np.empty(n, dtype=np.int32), "status": np.empty(n, dtype=np.int32)}
        ran = np.full(1, -1, dtype=np.int32)
        rc = self.lib.ikg_emu_project_paths(C.byref(self.md), C.byref(self.cd), q0.ctypes.data, A.ctypes.data,
                                            B.ctypes.data, n, float(step_size), int(max_nodes), g.ctypes.data, g.size,
                                            C.byref(self.prm), res["robot_path"].ctypes.data,
                                            res["cube_path"].ctypes.data, res["n_nodes"].ctypes.data,
                                            res["status"].ctypes.data, ran.ctypes.data)
        self.steps_run = int(ran[0])
        return rc, res

    def run(self, q0, A, B, step_size, max_nodes):
        rc, res = self.call(q0, A, B, step_size, max_nodes)
        assert rc == 0
        return res


@pytest.fixture(scope="module")
def emu():
    return Emu()


@pytest.fixture(scope="module")
def alone(emu):
    """Every chain alone at max_nodes = steps + 2, computed once."""
    return [pj.run_alone(emu.run, i) for i in range(len(pj.names()))]


def _placement(row):
    return row[:9].reshape(3, 3), row[9:]


# ---------------------------------------------------------------- the fixture
def test_fixture_covers_every_outcome(cases):
    c = cases
    st, nn, rot, pure = c["status"], c["n_nodes"], c["rotated"], c["pure_rotation"]
    assert len(pj.names()) == 17 and len(pj.group("main")) == 14 and len(pj.group("boundary")) == 3
    assert {int(s): int((st == s).sum()) for s in (0, 1, 2)} == {0: 10, 1: 2, 2: 5}
    assert ((st == 1) & (nn >= 3)).any() and ((st == 2) & (nn >= 3)).any()
    assert (rot & ~pure & (st == 0)).any() and (rot & (st == 1)).any()
    assert sorted(st[pure]) == [0, 2] and (c["steps"][pure] == 1).all()
    assert pj.longest(pj.group("main")) == 25
    # a chain that stops at its first step, one whose row 0 is no solution of its
    # placement (pathb: robot.q0), and the oracle's outcome table
    table = {n: (int(c["steps"][i]), int(nn[i]), int(st[i])) for i, n in enumerate(pj.names())}
    assert table == {"zero": (1, 2, 0), "short": (1, 2, 0), "obst": (6, 4, 1), "obst_rz": (6, 4, 1), "far": (25, 14, 2),
                     "up": (3, 3, 2), "down": (3, 1, 2), "rz": (9, 10, 0), "ryrz": (9, 10, 0), "half": (5, 6, 0),
                     "spin_m": (1, 2, 0), "spin_p": (1, 1, 2), "path": (9, 10, 0), "pathb": (13, 1, 2),
                     "b1": (2, 3, 0), "b4": (5, 6, 0), "b4s": (4, 5, 0)}
    # every chain's counts are consistent: reached = steps + 1 nodes, else fewer
    assert ((st == 0) == (nn == c["steps"] + 1)).all() and (nn <= c["steps"] + 1).all()
    assert np.array_equal(np.diff(c["row_off"]), nn)
    # one solve per accepted node, one more where the chain ended in a failed solve
    assert np.array_equal(np.diff(c["iters_off"]), nn - 1 + (st == 2))


def test_fixture_step_counts(cases):
    c = cases
    for i, name in enumerate(pj.names()):
        quot = np.linalg.norm(c["A"][i, 9:] - c["B"][i, 9:]) / c["step_size"][i]
        assert quot == c["quot"][i] and int(quot) + 1 == c["steps"][i]
        k = int(c["k"][i])
        if k < 0:
            assert quot == 0.0 or abs(quot - round(quot)) >= 1e-9, name
        elif name == "b4s":  # just below the integer: the device counts k steps, the host's allowance k + 1
            assert 0 < k - quot < 1e-11 and c["steps"][i] == k
            assert int(np.linalg.norm(c["A"][i, 9:] - c["B"][i, 9:]) / (c["step_size"][i] * (1.0 - 1e-12))) + 1 == k + 1
        else:
            # dyadic ends that differ on one axis by k 2^-5: every product, sum, root and quotient is exact
            assert c["step_size"][i] == 2.0 ** -5 and quot == float(k) and c["steps"][i] == k + 1, name
            d = (c["B"][i, 9:] - c["A"][i, 9:]) * 32
            assert np.count_nonzero(d) == 1 and abs(d).max() == k and (c["A"][i, 9:] * 32 == np.round(c["A"][i, 9:] * 32)).all()


def test_fixture_interpolation_and_placement_checks(cases, oscenes):
    """The recorded float64 rows are planner_oracle.se3_interpolate's, their
    recorded error is theirs against the 50-digit rows, and every deciding
    placement check answers the same on the inflated and the deflated scene."""
    from oracle import planner_oracle as po
    c = cases
    for i, name in enumerate(pj.names()):
        a, b = int(c["row_off"][i]), int(c["row_off"][i + 1])
        A, B = _placement(c["A"][i]), _placement(c["B"][i])
        steps, n = int(c["steps"][i]), b - a
        assert np.array_equal(c["cube_oracle"][a], c["A"][i]) and np.array_equal(c["cube_exact"][a], c["A"][i])
        deciding = list(range(1, n)) + ([n] if c["status"][i] == 1 else [])
        for s in deciding:
            R, t = po.se3_interpolate(A, B, s / steps)
            hit = [bool(po.target_env(oscenes[d], R, t)) for d in (0.0, DELTA, -DELTA)]
            assert hit == [s == n] * 3, (name, s, hit)
            if s < n:
                assert np.array_equal(np.concatenate([R.reshape(9), t]), c["cube_oracle"][a + s]), (name, s)
        assert np.array_equal(np.abs(c["cube_oracle"][a:b] - c["cube_exact"][a:b]).max(axis=1), c["cube_err"][a:b])
    assert c["cube_err"].max() <= 4 * np.finfo(float).eps


def test_fixture_solves_are_no_near_ties(cases, oscenes):
    """The recorded margins; the stops themselves are recomputed: each accepted
    row is collision-free on the inflated scene with both hand errors below
    eps (1 - 1e-6)."""
    from oracle import collision_oracle as co
    from oracle import ik_oracle as o
    c = cases
    acc = c["acc_err"]
    assert len(acc) == (c["n_nodes"] - 1).sum()
    assert (acc[:, 0] < EPS * (1 - TIE)).all()
    before = acc[~np.isnan(acc[:, 1]), 1]
    assert ((before > EPS * (1 + TIE)) | (before < EPS * (1 - TIE))).all()
    failing = c["status"] == 2
    assert np.array_equal(~np.isnan(c["fail_err"]), failing)
    assert ((c["fail_err"][failing] >= 2 * EPS) | c["fail_col"][failing]).all()
    # failing solves ran to max_iters; an accepted solve with 0 updates is the zero-length chain's
    for i, name in enumerate(pj.names()):
        it = c["iters"][int(c["iters_off"][i]):int(c["iters_off"][i + 1])]
        n = int(c["n_nodes"][i])
        assert (it[:n - 1] < 1000).all() and (not failing[i] or it[-1] == 1000), name
        assert (it[:n - 1] > 0).all() or name == "zero"
        a = int(c["row_off"][i])
        k = int(c["acc_off"][i])
        for s in range(1, n):
            R, t = _placement(c["cube_oracle"][a + s])
            eL, eR = o.hand_errors(c["q"][a + s], *o.hook_targets(R, t))
            assert max(np.linalg.norm(eL), np.linalg.norm(eR)) == acc[k + s - 1, 0], (name, s)
            assert not co.collision(oscenes[DELTA], c["q"][a + s], R, t), (name, s)


@pytest.mark.parametrize("name", [n for n in pj.names() if pj.cases()["status"][pj.index(n)] != 2])
def test_fixture_rows_reproduce_from_the_oracle(cases, oscenes, name):
    import warnings
    from oracle import planner_oracle as po
    c, i = cases, pj.index(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rp, cp = po.project_path(oscenes[0.0], c["q0"][i], _placement(c["A"][i]), _placement(c["B"][i]),
                                 float(c["step_size"][i]))
    q, _, _ = pj.rows(i)
    assert len(rp) == len(q) and np.array_equal(np.array(rp), q)
    a = int(c["row_off"][i])
    assert all(np.array_equal(np.concatenate([P[0].reshape(9), P[1]]), c["cube_oracle"][a + s]) for s, P in enumerate(cp))


# ---------------------------------------------------------------- the bookkeeping on the emulator
@pytest.mark.parametrize("name", pj.names())
def test_emulator_each_chain_alone(alone, name):
    i = pj.index(name)
    dq, ce = pj.compare(i, alone[i])
    print(f"{name}: |dq| vs oracle {dq:.2e}, cube-row error / bound {ce:.2f}")


@pytest.mark.parametrize("order", ["fixture", "reverse", "permuted"])
@pytest.mark.parametrize("which", ["main", "boundary"])
def test_emulator_one_call_mixed_outcomes(emu, alone, which, order):
    idx = {"fixture": pj.group(which), "reverse": pj.group(which)[::-1], "permuted": pj.permuted(which)}[order]
    res = pj.run_batch(emu.run, which, idx)
    assert sorted(set(int(s) for s in res["status"])) == ([0, 1, 2] if which == "main" else [0])
    for j, i in enumerate(idx):
        got = pj.chain_of(res, j)
        pj.compare(i, got)
        pj.same(got, alone[i])


def test_emulator_more_chains_than_a_block(emu, alone):
    """257 chains (two 256-thread blocks, nine waves of the solve): every copy is its chain's answer."""
    idx = pj.tiled("main", 257)
    res = pj.run_batch(emu.run, "main", idx)
    for j, i in enumerate(idx):
        pj.same(pj.chain_of(res, j), alone[i])
    assert (res["status"] != pj.LIVE).all()


def test_emulator_max_nodes_edges(emu):
    pj.check_max_nodes_edges(emu.run)


def test_emulator_step_boundary_and_spare_step(emu, alone, cases):
    c = cases
    for name in ("b1", "b4"):
        i = pj.index(name)
        k = int(c["k"][i])
        pj.run_alone(emu.run, i)
        assert emu.steps_run == k + 1 == c["steps"][i]
        assert (int(alone[i]["n_nodes"]), int(alone[i]["status"])) == (k + 2, pj.REACHED)
    # b4s: the chain is reached at step 4, the host's allowance runs a fifth, which must change nothing
    i = pj.index("b4s")
    got = pj.run_alone(emu.run, i)
    assert c["steps"][i] == 4 and emu.steps_run == 5
    pj.compare(i, got)
    # without room for the spare step (max_nodes - 1 = 4 steps) the same rows
    q0, A, B = pj.inputs([i])
    tight = pj.chain_of(emu.run(q0, A, B, pj.step_size("boundary"), 5), 0)
    assert emu.steps_run == 4
    pj.same(tight, got, tol=0.0)


def test_emulator_a_stopped_chain_idles_while_others_append(emu, alone, cases):
    """`down` stops at step 1 with one node, `obst` at step 4 with four, `far`
    goes on to step 14: each equals its answer alone, whatever its neighbours,
    and its rows past n_nodes stay zero through the later steps' commits."""
    idx = [pj.index(n) for n in ("down", "far", "obst", "spin_p", "far", "up", "path")]
    res = pj.run_batch(emu.run, "main", idx)
    assert emu.steps_run == 25
    for j, i in enumerate(idx):
        got = pj.chain_of(res, j)
        pj.compare(i, got)
        pj.same(got, alone[i], tol=0.0)


def test_emulator_refusals_leave_the_outputs(emu):
    q0, A, B = pj.inputs(pj.group("main")[:2])

    def filled(M):
        return {"robot_path": np.full((2, M, 15), 7.5), "cube_path": np.full((2, M, 12), 7.5),
                "n_nodes": np.full(2, 77, dtype=np.int32), "status": np.full(2, 77, dtype=np.int32)}

    far = B.copy()
    far[1, 9] += 3e7  # |dt| / step_size >= 1e9
    for kw in (dict(step_size=0.0), dict(step_size=-0.025), dict(max_nodes=0), dict(geoms=[emu.env[0], emu.target]),
               dict(B=far)):
        args = dict(q0=q0, A=A, B=B, step_size=0.025, max_nodes=4)
        args.update(kw)
        out = filled(4)
        rc, _ = emu.call(out=out, **args)
        assert rc == -1, kw
        assert all((v == (77 if v.dtype == np.int32 else 7.5)).all() for v in out.values()), kw
