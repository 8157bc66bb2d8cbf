"""The IK loop's carried joint trig at every step size and dt, on the device:
what tests/test_step_regime.py cannot reach through the host emulator -- the
wave-level selection between the short step, the longer series and the exact
sincos, the packed layout's arm coupling, the quad layout's own copy of the
rule, problems_per_wave, multi-start and the collision term's checkpoint,
resume and trajectory kernels.  Fixture: tests/golden/step_regime_cases.npz
(tests/golden/make_step_regime_golden.py).

Groups A and B: |q - q_mp| within the fixture's bucket bound (8 A 2^-53 fp64,
8 A 2^-24 fp32; the damped route against ik_oracle.computeqgrasppose(lam)).
Wave independence: a problem's bits do not depend on its wave-mates.  Group C
(whole solves): the gates of tests/test_gpu_parity.py, fp32 README's C3 gate.
Group D (collision term): the gates of tests/test_gpu_trig_update.py.
The tilted robot (tests/golden/step_regime_tilted.npz): the generic kernels,
pre-built and compiled at run time, against the 32-digit generic loop.

Measured |q - reference| / bound on the MI355X, largest per route: shared
q0 row, row per problem and problems_per_wave 1 and 7 0.08, quad fp64 0.05,
pair fp32 0.07 (group B 0.18), packed and quad fp32 0.07, damped 0.38, tilted
pre-built 0.11 (fp64) / 0.03 (fp32), hipRTC 0.08 / 0.03."""
import numpy as np
import pytest

import helpers
import step_regime_cases as sr
from ikgrasp import _lib

pytestmark = pytest.mark.gpu

PAIR, PACKED, QUAD = _lib.IKG_VARIANT_PAIR, _lib.IKG_VARIANT_PACKED, _lib.IKG_VARIANT_QUAD
# route -> (dtype, solve parameters, q0 mode).  q0 mode: "natural" passes the layout's own q0 (one
# shared row for "zero", a row per problem for "rows"); "bcast" always one shared row (a "rows"
# case then runs problem by problem); "rows" always a row per problem (the medium-range rule).
ROUTES = {
    "pair-f64-bcast": ("f64", dict(variant=PAIR), "bcast"),
    "pair-f64-rows": ("f64", dict(variant=PAIR), "rows"),
    "pair-f32": ("f32", dict(variant=PAIR), "natural"),
    "packed-f32": ("f32", dict(variant=PACKED), "natural"),
    "quad-f64": ("f64", dict(variant=QUAD), "natural"),
    "quad-f32": ("f32", dict(variant=QUAD), "natural"),
    "pair-f64-ppw1": ("f64", dict(variant=PAIR, ppw=1), "natural"),
    "pair-f64-ppw7": ("f64", dict(variant=PAIR, ppw=7), "natural"),
    "damped-f64": ("f64", dict(lam=sr.LAMBDA), "natural"),
}
FIELDS = ("q", "err", "iters", "converged")
Q_GATE, ERR_GATE = 1e-9, 1e-10  # tests/test_gpu_parity.py
EE_GATE = 1.4e-5                # README, C3: fp32 against the fp64 oracle's solution in end-effector space
BOX_GATE = 1e-12                # tests/test_gpu_trig_update.py: window boxes against full regeneration
# the collision term's damped route is held against the undamped oracle: lambda moves a
# converged q by about lambda itself (ik_oracle, 1e-6 -> 2e-7..9e-7, 1e-10 -> 2e-11..9e-11), so 1e-12
# keeps the damped kernel on its own code three decades under the 1e-9 gate
D_LAMBDA = 1e-12
REC_DOUBLES = 20  # values per record (ikg_solve.hpp record layout; bench.py collision_kernels)
# eps = 0 of the fixture's fixed update counts: the library asks for eps > 0, and this one's stop
# threshold on the squared norms (ikg_model_build.hpp stop_threshold) is the smallest subnormal
# (fp32: 0), which no iterate of these cases is below
NO_STOP = 1e-300
A_CASES = sr.a_cases()
A_IDS = ["{}-dt{}-K{}".format(*c) for c in A_CASES]


@pytest.fixture(scope="module")
def fx():
    return sr.load()


class Out:
    """The outputs of one or more launches, problem after problem; `rows` keeps those of each launch."""

    def __init__(self, parts, rows=slice(None)):
        for f in FIELDS:
            setattr(self, f, np.concatenate([np.asarray(getattr(p, f))[rows] for p in parts]))


def run(solver, route, tg, q0, **kw):
    """q0 [B, 15] rows, or None for q0 = 0.  -> Out with the route's outputs per problem."""
    dtype, extra, mode = ROUTES[route]
    tg = np.asarray(tg).reshape(-1, 12)
    B = len(tg)
    kw = dict(kw, dtype=dtype, **extra)
    if q0 is None and mode != "rows":
        return Out([solver.solve(tg, np.zeros(15), **kw)])
    q0 = np.zeros((B, 15)) if q0 is None else np.asarray(q0).reshape(B, 15)
    if mode == "bcast":
        return Out([solver.solve(tg[i:i + 1], q0[i], **kw) for i in range(B)])
    if B == 1:  # a [1, nq] q0 is read as the shared row: two copies of the problem select the per-row kernel
        s = solver.solve(np.concatenate([tg, tg]), np.concatenate([q0, q0]), **kw)
        assert all(np.array_equal(np.asarray(getattr(s, f))[0], np.asarray(getattr(s, f))[1]) for f in FIELDS)
        return Out([s], slice(0, 1))
    return Out([solver.solve(tg, q0, **kw)])


_DAMPED = {}


def damped_reference(tg, q0, dt, K):
    """ik_oracle.computeqgrasppose(lam) after exactly K updates; computed once per case."""
    from oracle import ik_oracle as o
    q0 = np.zeros((len(tg), 15)) if q0 is None else q0
    key = (tg.tobytes(), q0.tobytes(), dt, K)
    if key not in _DAMPED:
        _DAMPED[key] = np.array([o.computeqgrasppose(q0[i], t[:9].reshape(3, 3), t[9:], max_iters=K, dt=dt, eps=0.0,
                                                     lam=sr.LAMBDA)[0] for i, t in enumerate(tg)])
    return _DAMPED[key]


def _bound(fx, group, route, i):
    return float(fx[f"{group}_bound32" if ROUTES[route][0] == "f32" else f"{group}_bound64"][i])


def _layout_q0(fx, lay, key="a_q0_rows"):
    return None if lay == "zero" else fx[key]


def _same(a, i, b, j, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f)[i], getattr(b, f)[j]), (what, f)


# ---------------------------------------------------------------- groups A and B
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", range(len(A_CASES)), ids=A_IDS)
def test_group_a_within_bucket_bound(solver, fx, case, route):
    lay, dt, K = A_CASES[case]
    tg, q0 = fx["a_targets"], _layout_q0(fx, lay)
    g = run(solver, route, tg, q0, dt=dt, eps=NO_STOP, max_iters=K)
    assert not g.converged.any() and (g.iters == K).all()
    ref = damped_reference(tg, q0, dt, K) if route == "damped-f64" else fx["a_q_mp"][case]
    d, bound = float(np.abs(g.q.astype(np.float64) - ref).max()), _bound(fx, "a", route, case)
    print(f"{route} {lay} dt {dt} K {K}: |q - ref| = {d:.3e}, bound {bound:.3e}, ratio {d / bound:.3f}")
    assert d <= bound


@pytest.mark.parametrize("route", list(ROUTES))
def test_group_b_on_the_thresholds(solver, fx, route):
    """The first update lands 2^-20 (relative) below or above kIncMax / kIncMed of
    either precision, in a sum slot or a plain slot; the second consumes the
    advanced trig.  Whichever rule the kernel takes, the bucket bound holds."""
    worst, over = 0.0, []
    for i in range(len(fx["b_dt"])):
        tg, q0, dt = fx["b_targets"][i][None], fx["b_q0"][i][None], float(fx["b_dt"][i])
        g = run(solver, route, tg, q0, dt=dt, eps=NO_STOP, max_iters=sr.B_K)
        assert g.iters[0] == sr.B_K
        ref = damped_reference(tg, q0, dt, sr.B_K) if route == "damped-f64" else fx["b_q_mp"][i][None]
        d, bound = float(np.abs(g.q.astype(np.float64) - ref).max()), _bound(fx, "b", route, i)
        worst = max(worst, d / bound)
        if d > bound:
            over.append((i, float(fx["b_thr"][i]), int(fx["b_side"][i]), bool(fx["b_sum"][i]), d, bound))
    print(f"{route}: largest |q - ref| / bound over the 64 threshold cases {worst:.3f}")
    assert not over, over


@pytest.mark.parametrize("case", range(len(A_CASES)), ids=A_IDS)
def test_multistart_is_the_per_row_solve(solver, fx, case):
    """ikg_solve_multistart's answer for (target, seed) is the per-row solve's of
    that seed bit for bit (include/ikgrasp.h), and within the bucket bound of
    the 32-digit q where the fixture holds the pair."""
    lay, dt, K = A_CASES[case]
    kw = dict(dt=dt, eps=NO_STOP, max_iters=K, variant=PAIR)
    tg, bound = fx["a_targets"], float(fx["a_bound64"][case])
    if lay == "zero":  # 4 equal seeds x 8 targets, four times: every problem of the case
        for j in range(0, sr.N_A, 8):
            ms = solver.solve_multistart(tg[j:j + 8], np.zeros((4, 15)), **kw)
            per = solver.solve(tg[j:j + 8], np.zeros((8, 15)), **kw)
            _same(ms, slice(None), per, slice(None), (case, j))
            assert np.abs(ms.q - fx["a_q_mp"][case][j:j + 8]).max() <= bound
        return
    seeds, one = fx["a_q0_rows"][:4], []
    for s in range(4):  # every (target, seed): the seed twice (one seed alone is a shared q0 row: the other trig rule)
        ms = solver.solve_multistart(tg[:8], np.stack([seeds[s], seeds[s]]), **kw)
        assert (ms.best_seed == 0).all()
        per = solver.solve(tg[:8], np.tile(seeds[s], (8, 1)), **kw)
        _same(ms, slice(None), per, slice(None), (case, "seed", s))
        assert np.abs(ms.q[s] - fx["a_q_mp"][case][s]).max() <= bound  # (target s, seed s) is the fixture's problem s
        one.append(per)
    ms = solver.solve_multistart(tg[:8], seeds, **kw)  # 4 seeds x 8 targets: the best seed's answer
    for t in range(8):
        _same(ms, t, one[int(ms.best_seed[t])], t, (case, "best seed of target", t))


# ---------------------------------------------------------------- wave independence
# a shared q0 row runs a "rows" case problem by problem already: nothing to compare there
WAVE_CASES = [(lay, dt, r) for lay in sr.LAYOUTS for dt in sr.DTS for r in ROUTES if not (ROUTES[r][2] == "bcast" and lay == "rows")]


@pytest.mark.parametrize("lay,dt,route", WAVE_CASES, ids=["{}-dt{}-{}".format(*c) for c in WAVE_CASES])
def test_a_problem_does_not_see_its_wave_mates(solver, fx, lay, dt, route):
    """The 32 problems of a case (lanes in different regimes: the fixture's
    mixed waves) in one launch, with a 33rd (a wave holding one problem), in
    another lane order and each alone: the same bits."""
    K = max(sr.ks_for(dt))
    kw = dict(dt=dt, eps=NO_STOP, max_iters=K)
    tg, q0 = fx["a_targets"], _layout_q0(fx, lay)
    one = run(solver, route, tg, q0, **kw)
    plus = run(solver, route, np.concatenate([tg, tg[:1]]), None if q0 is None else np.concatenate([q0, q0[:1]]), **kw)
    _same(plus, slice(0, 32), one, slice(None), "B = 33 against B = 32")
    _same(plus, 32, one, 0, "the 33rd problem, alone in its wave")
    perm = (5 * np.arange(32) + 3) % 32
    moved = run(solver, route, tg[perm], None if q0 is None else q0[perm], **kw)
    _same(moved, slice(None), one, perm, "permuted batch")
    for i in range(32):
        alone = run(solver, route, tg[i:i + 1], None if q0 is None else q0[i:i + 1], **kw)
        _same(alone, 0, one, i, f"problem {i} alone")


# ---------------------------------------------------------------- group C: whole solves
C_ROUTES = ("pair-f64-bcast", "pair-f64-rows", "quad-f64", "packed-f32", "pair-f32", "quad-f32")


@pytest.mark.parametrize("route", C_ROUTES)
@pytest.mark.parametrize("case", range(2 * len(sr.C_DTS)))
def test_group_c_whole_solves(solver, fx, case, route):
    lay, dt = sr.LAYOUTS[fx["c_layout"][case]], float(fx["c_dt"][case])
    tg = fx["c_targets"]
    g = run(solver, route, tg, _layout_q0(fx, lay, "c_q0_rows"), dt=dt)
    ok, it, q, err = (fx["c_" + k][case] for k in ("converged", "iters", "q", "err"))
    if ROUTES[route][0] == "f32":
        assert np.array_equal(g.converged, ok) and (np.abs(g.iters.astype(int) - it) <= 1).all()
        hg, ho = solver.fk(g.q[ok].astype(np.float64)), solver.fk(q[ok])
        for h in range(2):
            e = helpers.se3_err(ho[:, h, :9].reshape(-1, 3, 3), ho[:, h, 9:], hg[:, h, :9].reshape(-1, 3, 3), hg[:, h, 9:])
            print(f"{route} {lay} dt {dt} hand {h}: end-effector distance to the oracle's solution {e.max():.3e}")
            assert e.max() <= EE_GATE
        return
    assert np.array_equal(g.converged, ok) and np.array_equal(g.iters, it)
    assert np.abs(g.q[ok] - q[ok]).max() <= Q_GATE
    assert np.abs(g.err[ok] - err[ok]).max() <= ERR_GATE


# ---------------------------------------------------------------- group D: the collision term
@pytest.fixture(scope="module")
def csolver():
    from ikgrasp.collision import load_nextage_scene
    from ikgrasp.solver import IKSolver
    s = IKSolver(device=0, scene=load_nextage_scene())
    yield s
    s.close()


@pytest.fixture(scope="module")
def d_one_launch(csolver, fx):
    return [csolver.solve(fx["d_targets"], np.zeros(15), dt=float(dt), check_collision=True) for dt in fx["d_dt"]]


def _d_gate(fx, k, sol, q_gate=Q_GATE):
    ok, conv0 = fx["d_converged"][k], fx["d_converged_plain"][k]
    cont = conv0 & ~ok  # converged but colliding at the first passing iterate: ran on
    assert ok.any() and cont.any() and (~conv0).any()
    assert np.array_equal(sol.converged, ok) and np.array_equal(sol.iters, fx["d_iters"][k])
    assert np.abs(sol.q[ok] - fx["d_q"][k][ok]).max() <= q_gate
    return ok, cont


@pytest.mark.parametrize("k", range(len(sr.D_DTS)))
def test_collision_term_against_oracle(csolver, fx, d_one_launch, k):
    sol = d_one_launch[k]
    ok, cont = _d_gate(fx, k, sol)
    assert np.abs(sol.err[ok] - fx["d_err"][k][ok]).max() <= ERR_GATE
    assert (sol.iters[cont] == 1000).all()
    assert np.abs(sol.err[cont] - fx["d_err"][k][cont]).max() <= Q_GATE
    tg = fx["d_targets"][cont]  # the iterate after max_iters: the kernel's collision test answers as on the oracle's q
    assert np.array_equal(csolver.collision(sol.q[cont], tg), csolver.collision(fx["d_q"][k][cont], tg))


@pytest.mark.parametrize("k", range(len(sr.D_DTS)))
def test_collision_windows_are_per_problem(csolver, fx, d_one_launch, k, monkeypatch):
    """One launch against two permuted halves and against records rounds of a
    1 MB budget bit for bit; every colliding problem's records regenerated
    (IKG_BOX_COVER=0) within 1e-12, and that in records rounds too: there every
    problem that collides at its first passing iterate is listed, more of them
    than the budget's record slots, so the rounds are several."""
    tg, dt, a = fx["d_targets"], float(fx["d_dt"][k]), d_one_launch[k]
    solve = lambda t: csolver.solve(t, np.zeros(15), dt=dt, check_collision=True)
    perm = np.random.default_rng(1).permutation(sr.N_D)
    for half in (perm[:32], perm[32:]):
        _same(solve(tg[half]), slice(None), a, half, "a permuted half")
    slots = (1 << 20) // (8 * REC_DOUBLES * (1000 + 1))  # bench.py collision_kernels: one listed problem's records
    listed = int((fx["d_converged_plain"][k] & ~fx["d_converged"][k]).sum())  # at least the problems that run on
    assert listed > slots >= 1
    monkeypatch.setenv("IKG_REC_BUDGET_MB", "1")
    _same(solve(tg), slice(None), a, slice(None), "records rounds")
    monkeypatch.setenv("IKG_BOX_COVER", "0")
    rounds = solve(tg)
    monkeypatch.delenv("IKG_REC_BUDGET_MB")
    c = solve(tg)
    _same(rounds, slice(None), c, slice(None), "records rounds, every colliding problem listed")
    assert np.array_equal(a.converged, c.converged) and np.array_equal(a.iters, c.iters)
    assert np.abs(a.q - c.q).max() <= BOX_GATE and np.abs(a.err - c.err).max() <= BOX_GATE


@pytest.mark.parametrize("route", ["quad-f64", "damped-f64"])
@pytest.mark.parametrize("k", range(len(sr.D_DTS)))
def test_collision_trajectory_kernel_routes(csolver, fx, k, route):
    """The routes without a checkpoint loop (the trajectory kernel) against the same oracle answer."""
    kw = dict(variant=QUAD) if route == "quad-f64" else dict(lam=D_LAMBDA)
    sol = csolver.solve(fx["d_targets"], np.zeros(15), dt=float(fx["d_dt"][k]), check_collision=True, **kw)
    _d_gate(fx, k, sol)


# ---------------------------------------------------------------- the tilted robot: generic kernels, pre-built and hipRTC
T_CASES = sr.t_cases()


@pytest.fixture(scope="module")
def tilted():
    """The tilted robot of tests/test_gpu_generic.py / test_gpu_jit.py on the pre-built generic
    kernels and on the kernels compiled against its tables at run time."""
    import os

    from ikgrasp.model import DualArmModel
    from ikgrasp.solver import IKSolver
    m = DualArmModel.from_urdf(os.path.join(sr.GOLDEN, "tilted_dualarm.urdf"), os.path.join(sr.GOLDEN, "tilted_cube.urdf"))
    pre, jit = IKSolver(m, device=0, specialize=False), IKSolver(m, device=0)
    jit.specialize("f64")
    jit.specialize("f32")
    assert jit.is_specialized("f64") and jit.is_specialized("f32") and not pre.is_specialized("f64")
    yield {"prebuilt": pre, "hiprtc": jit}
    pre.close()
    jit.close()


@pytest.fixture(scope="module")
def tfx():
    return sr.load_tilted()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("build", ["prebuilt", "hiprtc"])
@pytest.mark.parametrize("case", range(len(T_CASES)), ids=["dt{}-K{}".format(*c) for c in T_CASES])
def test_tilted_robot_within_bucket_bound(tilted, tfx, case, build, dtype):
    """trig_advance<T, IKG_GENERIC_MED> on joint steps, 16 problems with a q0 row each (8 from
    q0 = 0, 8 from the perturbed posture: lanes in different regimes), against the 32-digit
    generic loop within the bucket bound measured on generic_oracle.computeqgrasppose."""
    dt, K = T_CASES[case]
    g = tilted[build].solve(tfx["t_targets"], tfx["t_q0"], dtype=dtype, dt=dt, eps=NO_STOP, max_iters=K)
    assert not g.converged.any() and (g.iters == K).all()
    d = float(np.abs(g.q.astype(np.float64) - tfx["t_q_mp"][case]).max())
    bound = float(tfx["t_bound64" if dtype == "f64" else "t_bound32"][case])
    print(f"tilted {build} {dtype} dt {dt} K {K}: |q - q_mp| = {d:.3e}, bound {bound:.3e}, ratio {d / bound:.3f}")
    assert d <= bound


@pytest.mark.parametrize("build", ["prebuilt", "hiprtc"])
@pytest.mark.parametrize("dt", sr.DTS)
def test_tilted_problem_does_not_see_its_wave_mates(tilted, tfx, dt, build):
    K = max(k for d, k in T_CASES if d == dt)
    kw = dict(dt=dt, eps=NO_STOP, max_iters=K)
    tg, q0 = tfx["t_targets"], tfx["t_q0"]
    one = tilted[build].solve(tg, q0, **kw)
    for i in range(len(tg)):
        alone = tilted[build].solve(np.stack([tg[i], tg[i]]), np.stack([q0[i], q0[i]]), **kw)
        for f in FIELDS:
            assert np.array_equal(np.asarray(getattr(alone, f))[0], np.asarray(getattr(one, f))[i]), (i, f)
