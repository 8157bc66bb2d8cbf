"""GPU parity of the collision term: ikg_collision_batch and the
collision-continuation kernel against the collision oracle's fixtures
(tests/golden/collision_*.npz, made by tests/golden/make_golden.py).

Bars: collision booleans identical to the oracle on every fixture query
that is not within 1e-9 m (fp64) / 1e-4 m (fp32) of touching (flags
robust64/robust32, computed by re-running the oracle on inflated and deflated
geometry); solves with check_collision: identical success flags and update
counts, q within 1e-9 (fp64) of the oracle's loop.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csolver():
    from ikgrasp.collision import load_nextage_scene
    from ikgrasp.solver import IKSolver
    s = IKSolver(device=0, scene=load_nextage_scene())
    yield s
    s.close()


@pytest.fixture(scope="module")
def col_cases():
    return dict(np.load(os.path.join(GOLDEN, "collision_cases.npz")))


@pytest.fixture(scope="module")
def solve_cases():
    return dict(np.load(os.path.join(GOLDEN, "collision_solve_cases.npz")))


def _row(d):
    return np.concatenate([np.array(d["R"], dtype=np.float64).reshape(9), np.array(d["t"], dtype=np.float64)])


def test_collision_batch_fp64(csolver, col_cases):
    c = col_cases
    got = csolver.collision(c["q"], c["targets"])
    ok = c["robust64"].astype(bool)
    assert np.array_equal(got[ok], c["collision"][ok])
    assert got[0]  # KAT-5: collision(robot, robot.q0) is True


def test_collision_batch_fp32(csolver, col_cases):
    c = col_cases
    got = csolver.collision(c["q"], c["targets"], dtype="f32")
    ok = c["robust32"].astype(bool)
    assert np.array_equal(got[ok], c["collision"][ok])


def test_collision_batch_large_is_consistent(csolver, col_cases):
    """4096 queries (the fixture set tiled): same answers per copy."""
    c = col_cases
    reps = 4096 // len(c["q"]) + 1
    q = np.tile(c["q"], (reps, 1))[:4096]
    tg = np.tile(c["targets"], (reps, 1))[:4096]
    got = csolver.collision(q, tg)
    base = np.tile(csolver.collision(c["q"], c["targets"]), reps)[:4096]
    assert np.array_equal(got, base)


# continuation schedule: the default (trajectory first: ikg_traj_kernel's
# recorded iterates scanned by ikg_traj_scan_kernel), and the interleaved
# continuation (IKG_CONT_TRAJ=0, "0"), whose certified stretches run inside the
# continuation kernel
ROUNDS = [None, "0"]


def _schedule(monkeypatch, rounds):
    if rounds is not None:
        monkeypatch.setenv("IKG_CONT_TRAJ", "0")


@pytest.mark.parametrize("rounds", ROUNDS)
def test_solve_with_collision_fp64(csolver, solve_cases, oracle_cases, rounds, monkeypatch):
    _schedule(monkeypatch, rounds)
    c = solve_cases
    sol = csolver.solve(c["targets"], c["q0"], check_collision=True)
    assert np.array_equal(sol.converged, c["success"])
    assert np.array_equal(sol.iters, c["iters"])
    s = c["success"]
    assert np.abs(sol.q[s] - c["q"][s]).max() <= 1e-9
    assert np.abs(sol.err[s] - c["err"][s]).max() <= 1e-10
    cont = oracle_cases["converged"] & ~c["success"]  # converged but colliding -> ran on (:70)
    assert cont.sum() >= 5 and (sol.iters[cont] == 1000).all()
    # final iterate of those: same loop as the oracle (pinv drift only in the null space)
    assert np.abs(sol.err[cont] - c["err"][cont]).max() <= 1e-9
    # the final q collides (:97-98) for every failed-after-converging case
    assert csolver.collision(sol.q[cont], c["targets"][cont]).all()


@pytest.mark.parametrize("rounds", ROUNDS)
def test_solve_with_collision_fp32(csolver, solve_cases, rounds, monkeypatch):
    _schedule(monkeypatch, rounds)
    c = solve_cases
    sol = csolver.solve(c["targets"], c["q0"], dtype="f32", check_collision=True)
    # fp32 against the fp64 fixture: a success flag may flip only where the stop
    # test or the collision query is decided within fp32 rounding; the flips are
    # printed (pytest -s) so the count the gate allows is on record
    flips = np.nonzero(sol.converged != c["success"])[0]
    print(f"fp32 collision solves, schedule {rounds}: {len(flips)} of {len(sol.converged)} "
          f"success flags differ from the fp64 fixture: {flips.tolist()}")
    assert len(flips) <= 1  # measured 0 of 96 in every schedule (round 3)
    both = sol.converged & c["success"]
    assert (np.abs(sol.iters[both] - c["iters"][both]) <= 2).all()


def test_dropin_uses_collision_and_reproduces_kats(kat):
    import ikgrasp
    from ikgrasp.config import CUBE_PLACEMENT, CUBE_PLACEMENT_TARGET
    from ikgrasp.tools import collision
    robot, table, obstacle, cube = ikgrasp.setuppinocchio()
    assert robot.solver.scene is not None and table is not None and obstacle is not None
    assert collision(robot, robot.q0)  # KAT-5 (lab_instructions.ipynb:252)
    q0, ok0 = ikgrasp.computeqgrasppose(robot, robot.q0.copy(), cube, CUBE_PLACEMENT)
    qe, oke = ikgrasp.computeqgrasppose(robot, robot.q0.copy(), cube, CUBE_PLACEMENT_TARGET)
    assert ok0 and oke
    assert np.abs(q0 - kat["q0"]).max() <= 1e-12 and np.abs(qe - kat["qe"]).max() <= 1e-12
    assert not collision(robot, qe)


def test_multistart_with_collision_matches_single_solves(csolver, solve_cases, monkeypatch):
    c = solve_cases
    tg = c["targets"][:16]
    seeds = np.stack([np.zeros(15)] + [c["q0"][-k] for k in range(1, 4)])
    ms = csolver.solve_multistart(tg, seeds, check_collision=True)
    # a row per problem: the multi-start's trig rule (medium-range series), and
    # both record in the batch kernel (round 4): bit for bit
    per = [csolver.solve(tg, np.tile(s, (len(tg), 1)), check_collision=True) for s in seeds]
    for t in range(len(tg)):
        b = ms.best_seed[t]
        assert ms.converged[t] == per[b].converged[t]
        assert ms.converged[t] == any(p.converged[t] for p in per)
        assert ms.iters[t] == per[b].iters[t]
        assert np.array_equal(ms.q[t], per[b].q[t]) and np.array_equal(ms.err[t], per[b].err[t])
    # a broadcast seed: the exact-sincos rule for medium steps, so rounding only
    bc = [csolver.solve(tg, s, check_collision=True) for s in seeds]
    for t in range(len(tg)):
        b = ms.best_seed[t]
        assert ms.converged[t] == bc[b].converged[t] and ms.iters[t] == bc[b].iters[t]
        assert np.abs(ms.q[t] - bc[b].q[t]).max() <= 1e-9
    monkeypatch.setenv("IKG_TRAJ_REC", "0")
    per0 = [csolver.solve(tg, np.tile(s, (len(tg), 1)), check_collision=True) for s in seeds]
    ms0 = csolver.solve_multistart(tg, seeds, check_collision=True)
    for t in range(len(tg)):
        assert np.array_equal(ms0.q[t], per0[ms0.best_seed[t]].q[t])  # trajectory schedule: bit for bit


def test_multistart_packed_with_collision_matches_per_row_packed(csolver, solve_cases, monkeypatch):
    """a multi-start with variant PACKED and the collision term
    (the packed kernel records S > 1 seeds in the batch kernel) equals
    per-row packed solves of each seed bit for bit, and a broadcast seed too
    (fp32 takes the medium-range trig rule for every q0 layout); against the
    trajectory kernel (IKG_TRAJ_REC=0, which resyncs its trig per window) the
    flags and counts agree and q to fp32 rounding."""
    from ikgrasp import _lib
    c = solve_cases
    tg = c["targets"][:64]
    seeds = np.stack([np.zeros(15)] + [c["q0"][-k] for k in range(1, 4)])
    kw = dict(dtype="f32", check_collision=True, variant=_lib.IKG_VARIANT_PACKED)
    monkeypatch.setenv("IKG_TRAJ_REC", "1")
    ms = csolver.solve_multistart(tg, seeds, **kw)
    per = [csolver.solve(tg, np.tile(s, (len(tg), 1)), **kw) for s in seeds]
    bc = [csolver.solve(tg, s, **kw) for s in seeds]
    for t in range(len(tg)):
        b = ms.best_seed[t]
        for p in (per[b], bc[b]):
            assert ms.converged[t] == p.converged[t] and ms.iters[t] == p.iters[t]
            assert np.array_equal(ms.q[t], p.q[t]) and np.array_equal(ms.err[t], p.err[t])
    monkeypatch.setenv("IKG_TRAJ_REC", "0")
    ms0 = csolver.solve_multistart(tg, seeds, **kw)
    same = (ms0.converged == ms.converged) & (ms0.iters == ms.iters) & (ms0.best_seed == ms.best_seed)
    assert same.mean() >= 0.95, int((~same).sum())
    assert np.abs(ms0.q[same] - ms.q[same]).max() <= 1e-3


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_collision_answer_does_not_depend_on_q0_layout(csolver, solve_cases, dtype):
    """with the collision term, a broadcast q0 and a row per problem
    both record in the batch kernel (round 4), so from q0 = 0 the same problem
    gets the same bits either way; per-row runs of one seed equal the
    multi-start's (test above)."""
    c = solve_cases
    seed = c["q0"][0]
    assert not seed.any()
    a = csolver.solve(c["targets"], seed, dtype=dtype, check_collision=True)
    b = csolver.solve(c["targets"], np.tile(seed, (len(c["targets"]), 1)), dtype=dtype, check_collision=True)
    for x, y in zip((a.q, a.converged, a.iters, a.err), (b.q, b.converged, b.iters, b.err)):
        assert np.array_equal(x, y)


def test_check_collision_without_scene_fails_loudly(solver):
    from ikgrasp._lib import IkgError
    with pytest.raises(IkgError, match="collision scene"):
        solver.solve(np.concatenate([np.eye(3).reshape(9), [0.4, 0.1, 0.93]])[None], np.zeros(15),
                     check_collision=True)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_solve_with_collision_is_deterministic_at_bench_size(csolver, dtype):
    """C2's 4,096 uniform-sampler targets: the continuation's problem list is
    compacted in problem order and certificates only skip checks whose answer
    is known, so two solves agree bit for bit, and every problem reported
    successful is collision-free while every converged-but-failed one collides."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(4096, seed=0)
    a = csolver.solve(tg, np.zeros(15), dtype=dtype, check_collision=True)
    b = csolver.solve(tg, np.zeros(15), dtype=dtype, check_collision=True)
    assert np.array_equal(a.q, b.q) and np.array_equal(a.iters, b.iters)
    assert np.array_equal(a.converged, b.converged) and np.array_equal(a.err, b.err)
    free = csolver.solve(tg, np.zeros(15), dtype=dtype)
    ran_on = free.converged.astype(bool) & ~a.converged.astype(bool)
    assert a.converged.sum() > 0 and ran_on.sum() > 100
    ok = a.converged.astype(bool)
    free_ok = ~csolver.collision(a.q[ok], tg[ok], dtype=dtype)
    hit = csolver.collision(a.q[ran_on], tg[ran_on], dtype=dtype)
    if dtype == "f64":
        assert free_ok.all() and hit.all()
    else:  # fp32 GJK near touching contacts may answer differently by test order
        assert free_ok.mean() >= 0.99 and hit.mean() >= 0.99


def test_solve_with_collision_small_and_empty_batches(csolver, solve_cases):
    """B = 0, and single problems solved alone: same flags and update counts
    as inside the fixture batch, q equal to rounding (a problem's group-mates
    in the continuation only decide where its certified stretches pause, and a
    paused iterate is redone in the world frame: ulp-level differences)."""
    c = solve_cases
    empty = csolver.solve(np.zeros((0, 12)), np.zeros(15), check_collision=True)
    assert len(empty.q) == 0 and len(empty.converged) == 0
    full = csolver.solve(c["targets"], c["q0"], check_collision=True)
    for i in range(0, len(c["targets"]), max(1, len(c["targets"]) // 12)):
        one = csolver.solve(c["targets"][i:i + 1], c["q0"][i:i + 1], check_collision=True)
        assert one.converged[0] == full.converged[i] and one.iters[0] == full.iters[i]
        assert np.abs(one.q[0] - full.q[i]).max() <= 1e-12


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_trajectory_continuation_equals_interleaved(csolver, dtype, monkeypatch):
    """The trajectory-first continuation (default) and the interleaved one
    answer the same question -- the first iterate whose errors pass without
    collision -- on the same iterates: at C2's 4,096 uniform-sampler targets
    the flags and update counts agree (fp64: all; fp32: 99%) and q agrees to
    the rounding of the two FK formulations the iterates were computed with."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(4096, seed=0)
    a = csolver.solve(tg, np.zeros(15), dtype=dtype, check_collision=True)
    monkeypatch.setenv("IKG_CONT_TRAJ", "0")
    b = csolver.solve(tg, np.zeros(15), dtype=dtype, check_collision=True)
    same = (a.converged == b.converged) & (a.iters == b.iters)
    if dtype == "f64":
        assert same.all()
        assert np.abs(a.q - b.q).max() <= 1e-9
    else:
        assert same.mean() >= 0.99
        assert np.abs(a.q[same] - b.q[same]).max() <= 1e-3


def test_trajectory_continuation_windows(csolver, solve_cases, monkeypatch):
    """The records the pair kernel writes itself (IKG_TRAJ_REC=1, broadcast
    q0), the trajectory kernel's (default), and the latter in 16-iterate
    windows (several update/scan rounds, witnesses carried across them) give
    one answer."""
    c = solve_cases
    q0 = np.zeros(15)
    monkeypatch.setenv("IKG_TRAJ_REC", "1")
    a = csolver.solve(c["targets"], q0, check_collision=True)
    monkeypatch.setenv("IKG_TRAJ_REC", "0")
    b = csolver.solve(c["targets"], q0, check_collision=True)
    monkeypatch.setenv("IKG_TRAJ_WINDOW", "16")
    d = csolver.solve(c["targets"], q0, check_collision=True)
    for x in (b, d):
        assert np.array_equal(a.converged, x.converged) and np.array_equal(a.iters, x.iters)
        assert np.abs(a.q - x.q).max() <= 1e-9 and np.abs(a.err - x.err).max() <= 1e-12
    assert np.abs(b.q - d.q).max() <= 1e-12


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_records_in_batch_kernel_equal_trajectory_kernel(csolver, dtype, monkeypatch):
    """C2's 4,096 targets from q = 0: the batch kernel's own records (it keeps
    iterating past the first passing iterate) and the trajectory kernel's
    recomputed ones give the same flags and update counts."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(4096, seed=0)
    monkeypatch.setenv("IKG_TRAJ_REC", "1")
    a = csolver.solve(tg, np.zeros(15), dtype=dtype, check_collision=True)
    monkeypatch.setenv("IKG_TRAJ_REC", "0")
    b = csolver.solve(tg, np.zeros(15), dtype=dtype, check_collision=True)
    same = (a.converged == b.converged) & (a.iters == b.iters)
    if dtype == "f64":
        assert same.all() and np.abs(a.q - b.q).max() <= 1e-9
    else:
        assert same.mean() >= 0.99


@pytest.mark.parametrize("poison", ["0", "1"])
def test_packed_kernel_records_equal_trajectory_kernel(csolver, monkeypatch, poison):
    """The packed fp32 kernel writes the records itself (both arms' blocks from
    one lane) when they fit the budget: C2's 4,096 targets from q = 0 in the
    packed layout, its records against the trajectory kernel's recomputed ones
    (same flags and update counts; q to fp32 rounding: the trajectory kernel
    resyncs its trig per window), deterministic, and nothing read before it
    is written (IKG_POISON=1)."""
    from ikgrasp import _lib
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(4096, seed=0)
    monkeypatch.setenv("IKG_POISON", poison)
    monkeypatch.setenv("IKG_TRAJ_REC", "1")
    kw = dict(dtype="f32", check_collision=True, variant=_lib.IKG_VARIANT_PACKED)
    a = csolver.solve(tg, np.zeros(15), **kw)
    a2 = csolver.solve(tg, np.zeros(15), **kw)
    assert np.array_equal(a.q, a2.q) and np.array_equal(a.iters, a2.iters)
    monkeypatch.setenv("IKG_TRAJ_REC", "0")
    b = csolver.solve(tg, np.zeros(15), **kw)
    same = (a.converged == b.converged) & (a.iters == b.iters)
    print(f"packed records vs trajectory kernel: {int((~same).sum())} of 4096 differ in flag or count")
    assert same.mean() >= 0.999
    assert np.abs(a.q[same] - b.q[same]).max() <= 1e-3
    # converged without the collision term but not with it: ran on to max_iters (:70)
    free = csolver.solve(tg, np.zeros(15), dtype="f32", variant=_lib.IKG_VARIANT_PACKED)
    cont = free.converged & ~a.converged
    assert cont.sum() >= 100 and (a.iters[cont] == 1000).all()


@pytest.mark.parametrize("poison", ["0", "1"])
def test_trajectory_window_ending_at_max_iters(csolver, solve_cases, oracle_cases, monkeypatch, poison):
    """A record window that stops exactly at update max_iters without having
    recorded that iterate (k0 + m * Wn == max_iters) must hand it to the next
    window: the reference returns success = False at the iterate after
    max_iters updates (inverse_geometry.py:56, :97-98).  Every run-on fixture
    problem is solved alone with Wn = (1000 - k0) / m for m = 1, 2 where that
    is a whole window of >= 16; with IKG_POISON=1 every workspace starts as
    garbage, so a read of a slot this solve did not write shows up."""
    c = solve_cases
    monkeypatch.setenv("IKG_POISON", poison)
    cont = np.nonzero(oracle_cases["converged"] & ~c["success"])[0]
    assert len(cont) >= 5
    ran = 0
    for i in cont:
        k0 = int(oracle_cases["iters"][i])
        for mwin in (1, 2):
            if (1000 - k0) % mwin or (1000 - k0) // mwin < 16:
                continue
            monkeypatch.setenv("IKG_TRAJ_WINDOW", str((1000 - k0) // mwin))
            sol = csolver.solve(c["targets"][i:i + 1], c["q0"][i:i + 1], check_collision=True)
            assert not sol.converged[0] and sol.iters[0] == 1000, (i, k0, mwin)
            assert np.abs(sol.err[0] - c["err"][i]).max() <= 1e-9
            assert csolver.collision(sol.q, c["targets"][i:i + 1]).all()
            ran += 1
    assert ran >= 5


def test_poisoned_workspaces_give_the_same_answers(csolver, solve_cases, monkeypatch):
    """IKG_POISON=1 fills every stream-ordered workspace with garbage before
    use: each schedule of the continuation must still give the fixture answers
    (nothing is read before this solve writes it)."""
    c = solve_cases
    monkeypatch.setenv("IKG_POISON", "1")
    base = csolver.solve(c["targets"], c["q0"], check_collision=True)
    assert np.array_equal(base.converged, c["success"]) and np.array_equal(base.iters, c["iters"])
    for env in ({"IKG_TRAJ_REC": "1"}, {"IKG_TRAJ_WINDOW": "16"}, {"IKG_CONT_TRAJ": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sol = csolver.solve(c["targets"], c["q0"], check_collision=True)
        ref = base
        if "IKG_TRAJ_REC" in env:  # the batch kernel records for a broadcast q0 only
            sol = csolver.solve(c["targets"], np.zeros(15), check_collision=True)
            monkeypatch.setenv("IKG_TRAJ_REC", "0")
            ref = csolver.solve(c["targets"], np.zeros(15), check_collision=True)
        assert np.all(np.isfinite(sol.q)) and np.abs(sol.q).max() < 10, env
        assert np.array_equal(sol.converged, ref.converged) and np.array_equal(sol.iters, ref.iters), env
        for k in env:
            monkeypatch.delenv(k)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip((a.q, a.converged, a.iters, a.err), (b.q, b.converged, b.iters, b.err)))


def _close(a, b, tol):
    """Same flags and update counts; q and the hand errors within tol."""
    return (np.array_equal(a.converged, b.converged) and np.array_equal(a.iters, b.iters)
            and np.abs(a.q.astype(np.float64) - b.q).max() <= tol
            and np.abs(a.err.astype(np.float64) - b.err).max() <= tol)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_record_chunks_give_the_one_launch_answer(csolver, dtype, monkeypatch):
    """VERDICT r5 item 1 / ADVICE r5: a collision solve never draws on a shared
    pool, so a problem's answer does not depend on the chunking or on wave
    order.  C2's 4,096 targets: one launch with one records round (the default
    budgets); launch chunks whose checkpoints fit a 4 MB budget
    (IKG_CK_BUDGET_MB: fp64 ~230 problems per launch); records rounds of a
    4 MB records budget (IKG_REC_BUDGET_MB: fp64 26 listed problems per
    round) -- each solved twice, all bit for bit equal.  The same with every
    colliding problem's records regenerated (IKG_BOX_COVER=0)."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(4096, seed=0)
    kw = dict(dtype=dtype, check_collision=True)
    for env in ({}, {"IKG_BOX_COVER": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        one = csolver.solve(tg, np.zeros(15), **kw)
        for budget in ("IKG_CK_BUDGET_MB", "IKG_REC_BUDGET_MB"):
            monkeypatch.setenv(budget, "4")
            c1 = csolver.solve(tg, np.zeros(15), **kw)
            c2 = csolver.solve(tg, np.zeros(15), **kw)
            assert _same_bits(c1, c2), (env, budget)
            assert _same_bits(one, c1), (env, budget)
            monkeypatch.delenv(budget)
        for k in env:
            monkeypatch.delenv(k)
    assert 0 < int(one.converged.sum()) < 4096


@pytest.mark.parametrize("case", ["f64", "f32", "packed", "multistart"])
def test_window_boxes_agree_with_full_regeneration(csolver, solve_cases, monkeypatch, case):
    """VERDICT r5 item 2 (round 6): the batch kernel writes a checkpoint per
    32-iterate window from the first passing iterate on (ikg_solve.hpp kWin),
    not every iterate; the scan proves a colliding problem's windows by one
    certificate test on each window's box, and the windows it does not prove
    are regenerated from their checkpoints (the resume kernel) and scanned
    record by record.  IKG_BOX_COVER=0 proves no window, so every colliding
    problem is regenerated in full -- the round-5 records' work.  A problem
    whose windows are all proved takes the iterate after max_iters from the
    batch kernel's final record, a regenerated one from the resume kernel's
    records: the same loop compiled twice, so they agree to rounding (flags
    and update counts equal, q within 1e-12 fp64 / 1e-5 fp32), and each is
    deterministic (workspaces poisoned, solved twice).  Pair fp64, pair fp32,
    the packed fp32 layout and a multi-start."""
    from ikgrasp import _lib
    from ikgrasp.workload import uniform_targets
    monkeypatch.setenv("IKG_POISON", "1")
    tg = uniform_targets(4096, seed=0)
    tol = 1e-12 if case == "f64" or case == "multistart" else 1e-5
    if case == "multistart":
        c = solve_cases
        seeds = np.stack([np.zeros(15)] + [c["q0"][-k] for k in range(1, 4)])
        run = lambda: csolver.solve_multistart(tg[:1024], seeds, check_collision=True)
    else:
        kw = dict(dtype="f64" if case == "f64" else "f32", check_collision=True)
        if case == "packed":
            kw["variant"] = _lib.IKG_VARIANT_PACKED
        run = lambda: csolver.solve(tg, np.zeros(15), **kw)
    a = run()
    assert _same_bits(a, run())
    monkeypatch.setenv("IKG_BOX_COVER", "0")
    b = run()
    assert _same_bits(b, run())
    assert _close(a, b, tol)
    if case == "multistart":
        assert np.array_equal(a.best_seed, b.best_seed)
    else:
        assert 0 < int(a.converged.sum()) < 4096


@pytest.mark.parametrize("case", ["f64", "f32", "packed", "multistart"])
def test_split_scan_gives_the_one_wave_answer(csolver, solve_cases, monkeypatch, case):
    """The records scan deals a listed problem's 64-record chunks to G waves
    (IKG_SCAN_SPLIT: about that many waves in all, at most 8 per problem); the
    answer is the first collision-free passing record over all of them, written
    by the last wave to arrive.  It must be the one-wave scan's answer bit for
    bit: IKG_SCAN_SPLIT=0 (one wave per problem), the default, and 65,536 (8
    waves per problem), each solved twice with poisoned workspaces, also with
    every colliding problem regenerated (IKG_BOX_COVER=0: the most records)."""
    from ikgrasp import _lib
    from ikgrasp.workload import uniform_targets
    monkeypatch.setenv("IKG_POISON", "1")
    tg = uniform_targets(4096, seed=0)
    if case == "multistart":
        c = solve_cases
        seeds = np.stack([np.zeros(15)] + [c["q0"][-k] for k in range(1, 4)])
        run = lambda: csolver.solve_multistart(tg[:1024], seeds, check_collision=True)
    else:
        kw = dict(dtype="f64" if case == "f64" else "f32", check_collision=True)
        if case == "packed":
            kw["variant"] = _lib.IKG_VARIANT_PACKED
        run = lambda: csolver.solve(tg, np.zeros(15), **kw)
    for box in ("1", "0"):
        monkeypatch.setenv("IKG_BOX_COVER", box)
        monkeypatch.setenv("IKG_SCAN_SPLIT", "0")
        one = run()
        for split in ("2048", "65536"):
            monkeypatch.setenv("IKG_SCAN_SPLIT", split)
            a = run()
            assert _same_bits(a, run()), (box, split)
            assert _same_bits(one, a), (box, split)
            if case == "multistart":
                assert np.array_equal(one.best_seed, a.best_seed)
    assert 0 < int(one.converged.sum()) < one.converged.size


@pytest.mark.parametrize("case", ["f64", "f32", "packed"])
def test_collision_answers_keep_clamped_passive_joints(csolver, monkeypatch, case):
    """The passive head joints (tools.py:21-22: zero Jacobian columns) only
    move by the first update's clamp, so every answer of a collision solve --
    the first passing iterate, a later collision-free one, or the iterate
    after max_iters -- holds the clamped seed values.  The scan writes them
    from q_out (a full check's trig staging reuses the scratch the passive
    values were staged in); seeds outside the head limits make a wrong source
    visible.  Default scan, one wave per problem, and every colliding problem
    regenerated (IKG_BOX_COVER=0: the most full checks)."""
    from ikgrasp import _lib
    from ikgrasp.workload import uniform_targets
    from oracle import ik_oracle as o
    tg = uniform_targets(4096, seed=0)
    q0 = np.zeros(15)
    q0[1], q0[2] = 5.0, -5.0  # outside HEAD_JOINT0/1 limits
    kw = dict(dtype="f64" if case == "f64" else "f32", check_collision=True)
    if case == "packed":
        kw["variant"] = _lib.IKG_VARIANT_PACKED
    for env in ({}, {"IKG_SCAN_SPLIT": "0"}, {"IKG_BOX_COVER": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sol = csolver.solve(tg, q0, **kw)
        assert (sol.iters > 0).all()
        assert (sol.q[:, 1] == np.float32(o.UPPER[1]) if case != "f64" else sol.q[:, 1] == o.UPPER[1]).all(), env
        assert (sol.q[:, 2] == np.float32(o.LOWER[2]) if case != "f64" else sol.q[:, 2] == o.LOWER[2]).all(), env
        assert 0 < int(sol.converged.sum()) < 4096
        for k in env:
            monkeypatch.delenv(k)


def test_record_chunks_c3_fp32(csolver, monkeypatch):
    """C3 (65,536 fp32, packed layout) with the collision term: its checkpoints
    (570 MB) fit the default checkpoint budget in one launch and its listed
    problems' records take several rounds of the 1 GiB records budget; under a
    128 MB checkpoint budget the batch runs as 5 launch chunks, every chunk in
    the layout the whole batch resolves to (packed), and a 64 MB records budget
    takes ~80 rounds -- both give the one launch's bits."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(65536, seed=0)
    f = csolver.solve(tg, np.zeros(15), dtype="f32", check_collision=True)
    monkeypatch.setenv("IKG_CK_BUDGET_MB", "128")
    a = csolver.solve(tg, np.zeros(15), dtype="f32", check_collision=True)
    assert _same_bits(f, a)
    monkeypatch.delenv("IKG_CK_BUDGET_MB")
    monkeypatch.setenv("IKG_REC_BUDGET_MB", "64")
    b = csolver.solve(tg, np.zeros(15), dtype="f32", check_collision=True)
    assert _same_bits(f, b)


def test_multistart_record_chunks(csolver, solve_cases, monkeypatch):
    """A multi-start with the collision term splits over targets (each with its
    S seeds) when the checkpoints exceed their budget, and runs its records in
    rounds under a small records budget: 64 targets x 4 seeds with a 1 MB
    checkpoint budget (fp64: 15 targets per launch), then a 2 MB records
    budget, equal the one-launch answer."""
    c = solve_cases
    tg = c["targets"][:64]
    seeds = np.stack([np.zeros(15)] + [c["q0"][-k] for k in range(1, 4)])
    one = csolver.solve_multistart(tg, seeds, check_collision=True)
    for budget, mb in (("IKG_CK_BUDGET_MB", "1"), ("IKG_REC_BUDGET_MB", "2")):
        monkeypatch.setenv(budget, mb)
        ch = csolver.solve_multistart(tg, seeds, check_collision=True)
        assert _same_bits(one, ch) and np.array_equal(one.best_seed, ch.best_seed), budget
        monkeypatch.delenv(budget)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scan_certificates_do_not_change_answers(csolver, dtype, monkeypatch):
    """The records scan's inscribed-ball certificates (ikg_collision.hip
    scan_ball_cert / ball_covers) only skip narrow phases whose answer is
    "colliding": C2's 4,096 targets with the collision term give the same bits
    with them (IKG_SCAN_CERT=1) and without (0), with every colliding problem's
    records scanned (IKG_BOX_COVER=0, so the scan sees them all)."""
    from ikgrasp.workload import uniform_targets
    tg = uniform_targets(4096, seed=0)
    monkeypatch.setenv("IKG_BOX_COVER", "0")
    out = {}
    for c in ("1", "0"):
        monkeypatch.setenv("IKG_SCAN_CERT", c)
        out[c] = csolver.solve(tg, np.zeros(15), dtype=dtype, check_collision=True)
    a, b = out["1"], out["0"]
    for x, y in zip((a.q, a.converged, a.iters, a.err), (b.q, b.converged, b.iters, b.err)):
        assert np.array_equal(x, y)
    assert 0 < int(a.converged.sum()) < 4096
