"""Every evaluator of the SE(3) logarithm and exponential on the host emulator
(ikg_host_emu.hip ikg_emu_se3: the kernels' own functions in the kernels' own
instantiations) against 50-digit values (tests/se3_oracle.py, tests/golden/
se3_cases.npz), full vector, at the branch edges: the Taylor edge kPrec3 of both
dtypes, the alpha switch at pi/2, the near-pi edge pi - 1e-2, pi itself, the trace
clamps.  DESIGN.md "SE(3) log/exp accuracy by path" has the table.

  E1  log6<double>                 E2  log6<float>
  E3  log6<double, true> + exp6<double> (SE3.Interpolate; ikgrasp/se3.py is its host twin)
  E4  log6_iter<double>: no tracker / quad loop / pair loop / pair loop, z-aligned targets
  E5  log6_iter<float>             E6  log6_iter<v2f>

Gate (se3_oracle.gates): |got - exact| <= 16 ref_err[bucket], ref_err the reference
restatement's own error on the bucket's rows, with the floor 4 eps_T max(1, |p|) on v
and 4 eps_T max(1, theta) on w.  E1 and E4 between kPrec3 and pi - 1e-2 form
theta / (|skew|/2) with the acos angle and carry an envelope on top
(se3_oracle.envelope_gate): 4 K_meas eps / sin(theta) on w, and on v

  * "stated": 4 K_meas_v eps / sin(theta) |p|, the envelope of w times |p|, its constant measured
    like K_meas on the numpy restatement of the form.  K_meas_v = 4.55e3, not
    O(1): alpha = f/2 (1 + cos) carries f's RELATIVE error eps / sin^2(theta) and v = alpha p + ...,
    so eps / sin(theta) |p| is short by 1 / sin(theta), which the constant makes up at the smallest
    angle and over-allows above it (test_default_form_v_stated_envelope);
  * "derived": 4 Kv_meas eps / sin^2(theta) |p| (Kv_meas = 0.98), which follows the error over the
    band and is nowhere above the stated one: every other test here that needs E1's or E4's gate
    on v uses it.

Three shortcomings of log6_iter that this file found are pinned by strict xfails, each with
a passing test next to it that holds it to its size.
"""
import math

import numpy as np
import pytest

import emu as host_emu
import helpers
import se3_oracle as so

EPS = so.EPS["f64"]
RESYNC64 = 128  # Trig<double>::kResync (ikg_device.hpp)
KINC_ASIN = 0.035  # ThetaInc<double>::kIncAsin
CLAMP_HI, CLAMP_LO, PI_ID = 25, 26, 24  # angle ids of make_se3_golden.py

# name -> (ikg_emu_se3 fn, dtype, mid-band envelope)
EVALUATORS = {
    "E1": (0, "f64", True), "E2": (1, "f32", False), "E3": (2, "f64", False),
    "E4": (4, "f64", True), "E4-quad": (5, "f64", True), "E4-pair": (6, "f64", True), "E4-pair-z": (7, "f64", True),
    "E5": (8, "f32", False), "E6": (9, "f32", False),
}
LOOP = [k for k in EVALUATORS if k[:2] in ("E4", "E5", "E6")]
TRACKED = {"E4-quad": 5, "E4-pair": 6, "E4-pair-z": 7}


@pytest.fixture(scope="module")
def emu():
    lib = host_emu.load_or_skip()

    def run(fn, M, prev=None, width=6):
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1, 12)
        pv = None if prev is None else np.ascontiguousarray(prev, dtype=np.float64)
        out = np.full((len(M), width), np.nan)
        rc = lib.ikg_emu_se3(fn, len(M), M.ctypes.data, None if pv is None else pv.ctypes.data, out.ctypes.data)
        assert rc == 0, f"ikg_emu_se3({fn}) returned {rc}" + (": the packed halves differ" if rc == -2 else "")
        return out

    run.interpolate = host_emu.se3_interpolate
    return run


@pytest.fixture(scope="module")
def fx():
    return so.load()


@pytest.fixture(scope="module")
def results(emu, fx):
    """every evaluator over its dtype's rows, computed once: name -> (rows, got)"""
    out = {}
    for name, (fn, dtype, _) in EVALUATORS.items():
        rows = np.nonzero(fx["dtype"] == (0 if dtype == "f64" else 1))[0]
        out[name] = (rows, emu(fn, fx["M"][rows]))
    return out


def _symmetric(M):
    """rows whose R is exactly symmetric: |skew| = 0 (theta = pi, the tr < -1 clamp rows, and in
    fp32 the rows that round to such a matrix)"""
    return (M[:, 7] == M[:, 5]) & (M[:, 2] == M[:, 6]) & (M[:, 3] == M[:, 1]) & (M[:, 0] + M[:, 4] + M[:, 8] < 0)


def _bands(fx, rows, ratio, name):
    """worst error / gate per angle band, reported as the primitive tests do"""
    th, ai = fx["theta"][rows], fx["angle_id"][rows]
    dtype = EVALUATORS[name][1]
    bands = {"taylor": (th < so.PREC3[dtype]) & (ai < CLAMP_HI), "mid": so.mid_band(th, dtype) & (ai < CLAMP_HI),
             "near_pi": (th >= so.NEAR_PI) & (ai < CLAMP_HI), "clamps": ai >= CLAMP_HI}
    return {b: {"w": float(ratio[s, 3:].max()), "v": float(ratio[s, :3].max())} for b, s in bands.items()}


# ---------------------------------------------------------------- the gate, whole fixture
@pytest.mark.parametrize("name", list(EVALUATORS))
def test_evaluator_meets_its_gate(results, fx, name):
    """Every row, both sides of every edge, v and w; nothing but finite numbers on the clamp
    rows.  The loop evaluators' two pinned defects are left to their own tests below: v on
    the exactly symmetric rows, w on the tr < -1 clamp rows."""
    fn, dtype, env = EVALUATORS[name]
    rows, got = results[name]
    _, g = so.gates(fx, dtype, envelope="derived" if env else None)
    assert np.isfinite(got).all()
    err = np.abs(got - fx["exact"][rows])
    ratio = err / g
    if name in LOOP:
        ratio[_symmetric(fx["M"][rows]), :3] = 0.0
        ratio[fx["angle_id"][rows] == CLAMP_LO, 3:] = 0.0
    helpers.report(f"se3_emu_{name}", _bands(fx, rows, ratio, name))
    bad = np.nonzero((ratio > 1).any(axis=1))[0]
    assert len(bad) == 0, (name, "rows", rows[bad][:8], "theta", fx["theta"][rows][bad][:8], "err/gate", ratio[bad][:8])


def test_default_form_v_stated_envelope(results, fx):
    """E1 and E4, v between kPrec3 and pi - 1e-2 against w's envelope times |p|:
    16 ref_err + 4 K_meas_v (eps / sin theta) |p|, K_meas_v = 4.55e3 the worst err / (eps |p| /
    sin theta) of the numpy restatement of the form on the fixture's rows (make_se3_golden.py).
    With w's constant (K_meas = 1.00) in its place the kernels would miss it by 1.1e3 at 1.3e-4 rad
    (7.5e-8 absolute at |p| = 10), 3.0e2 at 2e-4 (1.1e-8), 84 at kPrec3 (6.1e-9), 8.3 at 1e-3
    (7.4e-11) and 17 at 1e-2 (2.1e-12), E1 and every E4 form alike: the error of v goes as
    eps / sin^2(theta) |p|, and test_evaluator_meets_its_gate holds the same rows to that."""
    worst = {}
    for name in ("E1", "E4", "E4-quad", "E4-pair", "E4-pair-z"):
        rows, got = results[name]
        _, g = so.gates(fx, "f64", envelope="stated")
        mid = so.mid_band(fx["theta"][rows]) & (fx["angle_id"][rows] < CLAMP_HI)
        ratio = (np.abs(got - fx["exact"][rows]) / g)[mid, :3].max(axis=1)
        th = fx["theta"][rows][mid]
        worst[name] = {f"{t:.6g}": float(ratio[th == t].max()) for t in np.unique(th)}
    helpers.report("se3_emu_stated_v_envelope", worst)
    assert max(max(w.values()) for w in worst.values()) <= 1.0, worst


# ---------------------------------------------------------------- log6_iter's two defects
def _loop_rows(results, fx, name, sel):
    rows, got = results[name]
    _, g = so.gates(fx, EVALUATORS[name][1], envelope="derived" if EVALUATORS[name][2] else None)
    s = sel(fx, rows)
    return rows[s], got[s], g[s]


@pytest.mark.parametrize("name", LOOP)
@pytest.mark.xfail(strict=True, reason="log6_iter: beta = 0 where |skew| = 0 (R exactly symmetric); DESIGN.md")
def test_loop_v_on_symmetric_rotations(results, fx, name):
    """theta = pi with sin = 0 exactly: v must meet the gate like any other row.  It does not:
    log6_iter takes 1/theta^2 from st q, q = 1 / max(theta^2 st, tiny), which is 0 at st = 0, so
    beta = (1 - alpha) / theta^2 comes out 0 and v loses beta (w.p) w -- |error| up to |p| (8.8
    at |p| = 10).  fp64: only R bitwise symmetric; fp32: also what rounds to it (pi - 1e-9)."""
    rows, got, g = _loop_rows(results, fx, name, lambda fx, r: _symmetric(fx["M"][r]))
    assert len(rows) >= 18
    assert (np.abs(got - fx["exact"][rows])[:, :3] <= g[:, :3]).all()


@pytest.mark.parametrize("name", LOOP)
def test_loop_v_on_symmetric_rotations_misses_one_term(results, fx, name):
    """The defect above is that one term and nothing else: v + (w.p) w / theta^2 meets the gate
    (plus the rounding of the term added here), w meets it as it stands."""
    rows, got, g = _loop_rows(results, fx, name, lambda fx, r: _symmetric(fx["M"][r]) & (fx["angle_id"][r] != CLAMP_LO))
    p, w = fx["M"][rows, 9:], got[:, 3:]
    term = (np.sum(w * p, axis=1) / np.sum(w * w, axis=1))[:, None] * w
    err = np.abs(got[:, :3] + term - fx["exact"][rows, :3])
    eps = so.EPS[EVALUATORS[name][1]]
    assert (err <= g[:, :3] + 4 * eps * np.abs(term).max(axis=1, keepdims=True)).all()
    assert (np.abs(got[:, 3:] - fx["exact"][rows, 3:]) <= g[:, 3:]).all()


@pytest.mark.parametrize("name", LOOP)
@pytest.mark.xfail(strict=True, reason="log6_iter: the tr < -1 clamp reaches theta but not the near-pi radicand; DESIGN.md")
def test_loop_w_on_the_low_clamp(results, fx, name):
    """tr < -1: Pinocchio clamps theta to pi and forms the axis with cos(theta - pi) = 1, so a
    diagonal entry of -1 gives a zero component.  log6_iter forms the radicand R_ii - c with the
    unclamped c = (tr - 1)/2 < -1, and the entry that was NOT nudged comes out as the root of the
    nudge."""
    rows, got, g = _loop_rows(results, fx, name, lambda fx, r: fx["angle_id"][r] == CLAMP_LO)
    assert len(rows) == 6
    assert (np.abs(got - fx["exact"][rows])[:, 3:] <= g[:, 3:]).all()


@pytest.mark.parametrize("name", LOOP)
def test_loop_w_on_the_low_clamp_is_the_root_of_the_nudge(results, fx, name):
    """... and no more than that: the radicand is at most (4 ulp) theta^2 / (1 - c), theta = pi,
    1 - c >= 2 (4.7e-8 measured in fp64, 1.1e-3 in fp32); finite, and the component along the
    axis within the gate."""
    rows, got, g = _loop_rows(results, fx, name, lambda fx, r: fx["angle_id"][r] == CLAMP_LO)
    eps = so.EPS[EVALUATORS[name][1]]
    err = np.abs(got - fx["exact"][rows])[:, 3:]
    assert np.isfinite(got).all()
    assert (err <= np.maximum(g[:, 3:], math.sqrt(4 * eps * math.pi ** 2 / 2) * (1 + 1e-3))).all()
    big = np.abs(fx["exact"][rows, 3:]) > 1
    assert (err[big] <= g[:, 3:][big]).all()
    # v on these rows: |skew| = 0, so it misses beta (w.p) w as on the other symmetric rows; with that term
    # put back it is off by what the spurious component of w (r) moves it, (1/2 + 2 theta beta) r |p| < 1.2 r |p|
    p, w = fx["M"][rows, 9:], got[:, 3:]
    term = (np.sum(w * p, axis=1) / np.sum(w * w, axis=1))[:, None] * w
    r = math.sqrt(4 * eps * math.pi ** 2 / 2)
    pn = np.linalg.norm(p, axis=1, keepdims=True)
    assert (np.abs(got[:, :3] + term - fx["exact"][rows, :3]) <= g[:, :3] + 1.2 * r * pn + 4 * eps * np.abs(term)).all()


# ---------------------------------------------------------------- exact properties
@pytest.mark.parametrize("name", list(EVALUATORS))
def test_signs_at_pi_are_the_references(results, fx, name):
    """theta = pi with an exactly zero skew part: every sign select is at a tie, where
    Pinocchio's `>` gives -; the sign bits (of zero components too) equal log6_ref's."""
    rows, got = results[name]
    s = fx["angle_id"][rows] == PI_ID
    assert s.sum() == 12 and _symmetric(fx["M"][rows][s]).all()
    assert np.array_equal(np.signbit(got[s, 3:]), np.signbit(fx["ref"][rows][s, 3:]))
    assert np.signbit(got[s, 3:]).all()


@pytest.mark.parametrize("name", list(EVALUATORS))
def test_identity_rotation_is_exact(results, fx, name):
    """R = 1 bitwise: w is exactly 0 and v is p bit for bit"""
    rows, got = results[name]
    s = fx["angle_id"][rows] == 0
    assert s.sum() == 28
    assert (got[s, 3:] == 0).all()
    assert np.array_equal(got[s, :3], fx["M"][rows][s, 9:])


def test_pair_and_packed_fp32_loops_agree_bitwise(results, fx):
    """E5 and E6 on the same float inputs (both take the angle from atan2_upper): identical bits"""
    assert np.array_equal(results["E5"][1].view(np.int64), results["E6"][1].view(np.int64))


def test_log6_accurate_is_accurate(fx):
    """se3_oracle.log6_accurate, which stands in for the 50 digits on the GPU: within
    8 eps max(1, |p|) of log6_mp on every row (2.1 measured).  The tr < -1 rows are left out:
    their `exact` is another matrix's, the un-nudged one's."""
    s = fx["angle_id"] != CLAMP_LO
    err = np.abs(so.log6_accurate(fx["M"][s]) - fx["exact"][s]).max(axis=1)
    bound = 8 * EPS * np.maximum(1.0, np.linalg.norm(fx["M"][s, 9:], axis=1))
    print("log6_accurate: worst err / (eps max(1, |p|))", (8 * err / bound).max())
    assert (err <= bound).all()


# ---------------------------------------------------------------- E3: log, exp, interpolation
def _exp_gate(fx):
    re = fx["exp_ref_err"][fx["exp_angle_id"]]
    vn = np.linalg.norm(fx["exp_xi"][:, :3], axis=1)
    return np.maximum(16 * re[:, 0], 4 * EPS), np.maximum(16 * re[:, 1], 4 * EPS * np.maximum(1.0, vn))


def _interp_gate(fx):
    re = fx["interp_ref_err"][fx["interp_angle_id"]]
    tn = np.linalg.norm(fx["interp_exact"][:, 9:], axis=1)
    return np.maximum(16 * re[:, 0], 4 * EPS), np.maximum(16 * re[:, 1], 4 * EPS * np.maximum(1.0, tn))


def _within(got, exact, gR, gt):
    err = np.abs(got - exact)
    return float((err[:, :9].max(axis=1) / gR).max()), float((err[:, 9:].max(axis=1) / gt).max())


def _flat(x):
    return np.concatenate([x.rotation.reshape(9), x.translation])


def test_exp6_meets_its_gate(emu, fx):
    """exp6<double> (the emulator) and ikgrasp.se3.exp6, both sides of its own Taylor edge included"""
    from ikgrasp import se3
    gR, gt = _exp_gate(fx)
    xi = np.concatenate([fx["exp_xi"], np.zeros_like(fx["exp_xi"])], axis=1)
    worst = {"emu": _within(emu(3, xi, width=12), fx["exp_exact"], gR, gt),
             "se3.py": _within(np.array([_flat(se3.exp6(x)) for x in fx["exp_xi"]]), fx["exp_exact"], gR, gt)}
    helpers.report("se3_emu_exp6", worst)
    assert max(max(w) for w in worst.values()) <= 1.0, worst


def test_interpolate_meets_its_gate(emu, fx):
    """se3_interpolate (log6<double, true> then exp6<double>) on the emulator and
    ikgrasp.se3.interpolate, the host route of project_paths: within 16x the float64
    restatement's own error of the 50-digit placement; alpha = 0 returns A within the floor,
    alpha = 1 returns B within the gate."""
    from ikgrasp import se3
    A, B, al = fx["interp_A"], fx["interp_B"], fx["interp_alpha"]
    gR, gt = _interp_gate(fx)
    got = emu.interpolate(A, B, al)
    host = np.array([_flat(se3.interpolate(a, b, c)) for a, b, c in zip(A, B, al)])
    worst = {"emu": _within(got, fx["interp_exact"], gR, gt), "se3.py": _within(host, fx["interp_exact"], gR, gt)}
    helpers.report("se3_emu_interpolate", worst)
    assert max(max(w) for w in worst.values()) <= 1.0, worst
    for o in (got, host):
        a0, a1 = al == 0.0, al == 1.0
        floor = 4 * EPS * np.maximum(1.0, np.linalg.norm(A[a0, 9:], axis=1))
        assert (np.abs(o[a0] - A[a0]).max(axis=1) <= floor).all()
        assert max(_within(o[a1], B[a1], gR[a1], gt[a1])) <= 1.0


def test_host_log6_meets_the_interpolation_gate(fx):
    """ikgrasp.se3.log6 (Pinocchio's own form): the E3 gate, no envelope"""
    from ikgrasp import se3
    rows, g = so.gates(fx, "f64")
    got = np.array([se3.log6(m) for m in fx["M"][rows]])
    assert np.isfinite(got).all() and (np.abs(got - fx["exact"][rows]) <= g).all()


# ---------------------------------------------------------------- the tracked angle
CHAIN_STARTS = (3e-4, 1e-2, 1.0, math.pi - 2e-2, math.pi - 5e-3, "rising")
STEPS = RESYNC64 - 1


def _rot(axis, theta):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(theta * axis / np.linalg.norm(axis)).as_matrix()


@pytest.fixture(scope="module")
def chains(fx):
    """Per start angle and axis motion: STEPS + 1 placements about a fixed or a slowly turning
    axis, the angle scaled by 0.99 per step (one IK update at dt = 1e-2), or rising from
    pi - 1.5e-2 through pi - 1e-2 to pi - 5e-3; |p| = 1.  With the 50-digit log of every row,
    the reference's own error over the chain and the rows' gate."""
    rng = np.random.default_rng(5)
    out = {}
    for start in CHAIN_STARTS:
        for turning in (False, True):
            ax, dax = rng.normal(size=3), rng.normal(size=3) * 2e-3
            th = math.pi - 1.5e-2 if start == "rising" else start
            scale = (1 + 1e-2 / th) ** (1.0 / STEPS) if start == "rising" else 0.99
            M = []
            for k in range(STEPS + 1):
                p = rng.normal(size=3)
                M.append(np.concatenate([_rot(ax + k * dax * turning, th).reshape(9), p / np.linalg.norm(p)]))
                th *= scale
            M = np.array(M)
            exact = np.array([so.log6_mp(m) for m in M])
            ref = np.array([so.log6_ref(m) for m in M])
            theta, pn = np.linalg.norm(exact[:, 3:], axis=1), np.linalg.norm(M[:, 9:], axis=1)
            re = np.abs(ref - exact)
            g = np.empty((len(M), 6))
            g[:, :3] = np.maximum(16 * re[:, :3].max(), 4 * EPS * np.maximum(1.0, pn))[:, None]
            g[:, 3:] = np.maximum(16 * re[:, 3:].max(), 4 * EPS * np.maximum(1.0, theta))[:, None]
            floor = np.empty((len(M), 6))
            floor[:, :3] = (4 * EPS * np.maximum(1.0, pn))[:, None]
            floor[:, 3:] = (4 * EPS * np.maximum(1.0, theta))[:, None]
            out[(start, turning)] = dict(M=M, exact=exact, theta=theta, pn=pn, floor=floor,
                                         gate=g + so.envelope_gate(fx, theta, pn, "derived"))
    return out


def _drift(fx, c):
    """What the tracked angle may add to a row's error after k increments from the resync row 0:
    that row's own angle error, K_meas eps / sin(theta_0) (acos, at either end of its range), and
    k roundings of the running sum, eps max(1, theta) each.  On w as it stands; on v through
    alpha, by |p| / sin(theta) inside the mid band and |p| beyond."""
    th, k = c["theta"], np.arange(len(c["theta"]))
    dth = 4 * float(fx["K_meas"]) * EPS / math.sin(th[0]) + k * EPS * max(1.0, th.max())
    d = np.empty((len(th), 6))
    d[:, 3:] = dth[:, None]
    d[:, :3] = (dth * c["pn"] / np.where(so.mid_band(th), np.sin(th), 1.0))[:, None]
    return d


@pytest.mark.parametrize("name", list(TRACKED))
def test_tracked_angle_over_a_resync_period(emu, fx, chains, name):
    """kResync - 1 increments with no resync, every step's full e[6] within the row's E4 gate (v at
    the derived envelope): worst 0.14, on the turning chain from 3e-4 rad."""
    worst = {}
    for key, c in chains.items():
        got = emu(TRACKED[name] + 10, c["M"][1:], prev=c["M"][:1])
        assert np.isfinite(got).all()
        ratio = np.abs(got - c["exact"][1:]) / c["gate"][1:]
        worst[f"{key[0]}{'-turning' if key[1] else ''}"] = float(ratio.max())
    helpers.report(f"se3_emu_tracked_{name}", worst)
    assert max(worst.values()) <= 1.0, worst


def _excess(emu, chains, start):
    """per row of `start`'s two chains and tracked form: (tracked error - exact-angle error, chain)"""
    for turning in (False, True):
        c = chains[(start, turning)]
        for fn in TRACKED.values():
            tr = np.abs(emu(fn + 10, c["M"][1:], prev=c["M"][:1]) - c["exact"][1:])
            un = np.abs(emu(fn, c["M"][1:]) - c["exact"][1:])
            yield tr - un, c


# where the tracked step is more than a floor worse than the exact-angle call: every start but 1 rad
# starts whose resync row lies where acos is worse than on the rows that follow: towards pi
_CARRIED = pytest.mark.xfail(strict=True, reason="log6_iter: the tracked angle keeps its resync row's acos error; DESIGN.md")
_FROM_NEAR_PI = (math.pi - 2e-2, math.pi - 5e-3)


@pytest.mark.parametrize("start", [pytest.param(s, marks=_CARRIED if s in _FROM_NEAR_PI else ()) for s in CHAIN_STARTS])
def test_tracked_increment_no_worse_than_the_exact_angle(emu, fx, chains, start):
    """The increment must not make a step worse than the exact-angle call on the same row by
    more than the floor (4 eps max(1, |p|) on v, 4 eps max(1, theta) on w) -- the exact call
    taken at its envelope where it has one: inside the mid band its own error varies from row to
    row between 0 and eps / sin(theta) (eps |p| / sin^2(theta) on v), so a difference of the two
    errors below that says nothing about the tracker (from 3e-4 rad the tracked step is 2.6e6 floors
    worse than the exact one on some rows and as much better on others).

    Held from 3e-4, 1e-2 and 1 rad and on the rising chain (at most 0.5 floors over all 127 steps;
    at 1 rad with no envelope to lean on).  On the chains that come down from near pi the resync
    row's acos error, eps / sin(pi - 5e-3) = 4.4e-14, is kept down to rows where the exact call has
    far less: 26 floors from pi - 5e-3, 5.6 from pi - 2e-2.  test_tracked_increment_excess_is_the_carried_error holds that excess to its size."""
    worst = 0.0
    for d, c in _excess(emu, chains, start):
        over = d - so.envelope_gate(fx, c["theta"], c["pn"], "derived")[1:]
        worst = max(worst, float((over / c["floor"][1:]).max()))
    helpers.report(f"se3_emu_tracked_vs_exact_floors_{start}", {"floors": worst})
    assert worst <= 1.0, worst


@pytest.mark.parametrize("start", CHAIN_STARTS)
def test_tracked_increment_excess_is_the_carried_error(emu, fx, chains, start):
    """... and what the tracked step is worse by is no more than the floor, the exact-angle call's
    own envelope on that row and what the construction carries along (_drift: the resync row's
    acos error, one rounding per increment)."""
    for d, c in _excess(emu, chains, start):
        allowed = c["floor"] + _drift(fx, c) + so.envelope_gate(fx, c["theta"], c["pn"], "derived")
        assert (d <= allowed[1:]).all(), (start, float((d / allowed[1:]).max()))


@pytest.mark.parametrize("name", list(TRACKED))
def test_large_step_falls_back_to_the_exact_angle(emu, name):
    """A step of more than kIncAsin in the angle's sine: the tracker must discard its increment,
    and the result is the resync call's bit for bit; a small step differs from it only within
    rounding (so the tracked path did run there)."""
    rng = np.random.default_rng(6)
    M, big, small = [], [], []
    for th in (3e-4, 0.5, 1.0, 2.0, 3.0, math.pi - 5e-3):
        ax, p = rng.normal(size=3), rng.normal(size=3)
        M.append(np.concatenate([_rot(ax, th).reshape(9), p]))
        for prev, d in ((big, 1.5 * KINC_ASIN), (big, -1.2 * KINC_ASIN), (small, 0.5 * KINC_ASIN)):
            prev.append(np.concatenate([_rot(ax, abs(th + d)).reshape(9), p]))
    M = np.array(M)
    exact = emu(TRACKED[name], M)
    got = emu(TRACKED[name], np.repeat(M, 2, axis=0), prev=np.array(big))
    assert np.array_equal(got.view(np.int64), np.repeat(exact, 2, axis=0).view(np.int64))
    near = emu(TRACKED[name], M, prev=np.array(small))
    assert not np.array_equal(near, exact) and np.abs(near - exact).max() <= 1e-6
