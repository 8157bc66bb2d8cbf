"""The robot family (tests/robot_family.py) on the GPU: every model
specialisation -- kSpecNextage on robots that are not the Nextage,
kSpecGenericWrist, kSpecGeneric (the 6x6 Householder QR) -- through the
prebuilt kernels and through the hipRTC-compiled ones, against the raw-axis
oracle's fixtures (tests/golden/family_cases.npz, oracle/generic_oracle.py).

Tolerances, the project's (test_gpu_generic.py, test_gpu_jit.py,
test_gpu_control.py): fp64 -- identical flags and update counts, converged q
within 1e-9 and err within 1e-10 of the oracle, the specialised kernel within
1e-11 of the prebuilt one, FK / frame terms within 1e-12; fp32 -- identical
flags, counts within +-2, hand SE(3) distance to the fp64 fixture <= 1e-4,
frame terms within 2e-4.  Every check prints its largest error."""
import os
import time

import numpy as np
import pytest

import emu as host_emu
import robot_family as rf
from helpers import se3_err

pytestmark = pytest.mark.gpu

PAIR, PACKED, QUAD, AUTO = 1, 2, 3, 0
NX = ("nx_scaled", "nx_extra_zero")  # kSpecNextage members: the Nextage-only kernels
JIT32 = ("nx_scaled", "offset_wrist", "mixed_axes")  # fp32 is compiled for these only (compile time)
KEYS = ("placement", "velocity", "J", "dJ", "dJv")
T0 = time.time()


@pytest.fixture(scope="module")
def cases():
    return rf.load_cases()


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    """name -> (specialised, prebuilt) solvers, made on first use and kept for
    the module; code objects are cached within the run."""
    from ikgrasp.solver import IKSolver
    old = os.environ.get("IKG_JIT_CACHE_DIR")
    os.environ["IKG_JIT_CACHE_DIR"] = str(tmp_path_factory.mktemp("ikg_jit"))
    made = {}

    def get(name):
        if name not in made:
            m = rf.load_model(name)
            made[name] = (IKSolver(m, device=0), IKSolver(m, device=0, specialize=False))
            t = time.time()
            made[name][0].specialize("f64")  # raises when the compile fails: no silent fall-back
            print(f"{name}: hipRTC f64 {time.time() - t:.1f} s")
        return made[name]

    yield get
    for pair in made.values():
        for s in pair:
            s.close()
    if old is None:
        del os.environ["IKG_JIT_CACHE_DIR"]
    else:
        os.environ["IKG_JIT_CACHE_DIR"] = old
    print(f"test_gpu_robot_family: {time.time() - T0:.1f} s wall")


def _same(a, b, tol=1e-11):
    """test_gpu_jit.py's _same: specialised vs prebuilt."""
    assert np.array_equal(a.converged, b.converged) and np.array_equal(a.iters, b.iters)
    ok = b.converged
    d = float(np.abs(a.q[ok] - b.q[ok]).max()) if ok.any() else 0.0
    assert d <= tol, d
    return d


def _vs_oracle64(tag, sol, q, conv, iters, err=None):
    ok = conv.astype(bool)
    same = np.array_equal(sol.converged, ok) and np.array_equal(sol.iters, iters)
    dq = float(np.abs(sol.q[ok] - q[ok]).max()) if same else float("nan")
    de = float(np.abs(sol.err[ok] - err[ok]).max()) if same and err is not None else 0.0
    print(f"{tag}: flags/counts {'equal' if same else 'DIFFER'}, |dq| {dq:.2e}, |derr| {de:.2e}")
    assert same, (sol.converged.tolist(), sol.iters.tolist(), iters.tolist())
    assert dq <= 1e-9 and de <= 1e-10


def _vs_oracle32(tag, solver, sol, q, conv, iters):
    ok = conv.astype(bool)
    flags = np.array_equal(sol.converged, ok)
    dit = int(np.abs(sol.iters[ok].astype(int) - iters[ok]).max())
    h32, h64 = solver.fk(sol.q[ok].astype(np.float64)), solver.fk(q[ok])
    e = max(float(se3_err(h32[:, h, :9].reshape(-1, 3, 3), h32[:, h, 9:], h64[:, h, :9].reshape(-1, 3, 3),
                          h64[:, h, 9:]).max()) for h in range(2))
    print(f"{tag}: flags {'equal' if flags else 'DIFFER'}, count difference {dit}, hand SE(3) distance {e:.2e}")
    assert flags, sol.converged.tolist()
    assert dit <= 2 and e <= 1e-4


# ---------------------------------------------------------------- per member
@pytest.mark.parametrize("name", rf.NAMES)
def test_specialize_compiles(family, name):
    """The member's Spec<PAT, PROT, WRIST, ZMASK> instantiation compiles (a
    failure raises in the fixture) and is in use."""
    jit, pre = family(name)
    assert jit.is_specialized("f64") and not pre.is_specialized("f64")


@pytest.mark.parametrize("name", rf.NAMES)
def test_fp64_matches_oracle_prebuilt_and_jit(family, cases, name):
    jit, pre = family(name)
    c = cases[name]
    # per-problem seeds (the medium-range trig loop), then the broadcast q0 = 0 seed on the cold cases
    for tag, tg, q0, sl in (("seeds", c["targets"], c["q0"], slice(None)),
                            ("broadcast", c["targets"][:8], np.zeros(jit.nq), slice(0, 8))):
        a, b = jit.solve(tg, q0), pre.solve(tg, q0)
        _vs_oracle64(f"{name} fp64 prebuilt {tag}", b, c["q"][sl], c["converged"][sl], c["iters"][sl], c["err"][sl])
        _vs_oracle64(f"{name} fp64 jit {tag}", a, c["q"][sl], c["converged"][sl], c["iters"][sl], c["err"][sl])
        print(f"{name} fp64 jit vs prebuilt {tag}: {_same(a, b):.2e}")
    assert not pre.is_specialized("f64")


@pytest.mark.parametrize("name", rf.NAMES)
def test_fp32_prebuilt(family, cases, name):
    _, pre = family(name)
    c = cases[name]
    _vs_oracle32(f"{name} fp32 prebuilt", pre, pre.solve(c["targets"], c["q0"], dtype="f32"), c["q"], c["converged"], c["iters"])
    assert not pre.is_specialized("f32")


@pytest.mark.parametrize("name", JIT32)
def test_fp32_jit(family, cases, name):
    jit, _ = family(name)
    c = cases[name]
    t = time.time()
    jit.specialize("f32")
    print(f"{name}: hipRTC f32 {time.time() - t:.1f} s")
    assert jit.is_specialized("f32")
    _vs_oracle32(f"{name} fp32 jit", jit, jit.solve(c["targets"], c["q0"], dtype="f32", variant=PAIR), c["q"],
                 c["converged"], c["iters"])


# ---------------------------------------------------------------- the Nextage-only kernels on other robots
@pytest.mark.parametrize("variant", [PAIR, QUAD, AUTO])
@pytest.mark.parametrize("name", NX)
def test_nextage_class_variants_fp64(family, cases, name, variant):
    """Frame-1 closed form, the medium-range trig series (per-problem seeds)
    and the short one (broadcast), the QUAD layout and the in-kernel constants:
    nothing may carry a Nextage length, hand angle or limit."""
    c = cases[name]
    for which, s in zip(("jit", "prebuilt"), family(name)):
        _vs_oracle64(f"{name} fp64 variant {variant} {which} seeds", s.solve(c["targets"], c["q0"], variant=variant),
                     c["q"], c["converged"], c["iters"], c["err"])
        _vs_oracle64(f"{name} fp64 variant {variant} {which} broadcast",
                     s.solve(c["targets"][:8], np.zeros(s.nq), variant=variant), c["q"][:8], c["converged"][:8],
                     c["iters"][:8], c["err"][:8])


@pytest.mark.parametrize("variant", [PAIR, PACKED, AUTO])
@pytest.mark.parametrize("name", NX)
def test_nextage_class_variants_fp32(family, cases, name, variant):
    _, pre = family(name)
    c = cases[name]
    _vs_oracle32(f"{name} fp32 variant {variant} seeds", pre, pre.solve(c["targets"], c["q0"], dtype="f32", variant=variant),
                 c["q"], c["converged"], c["iters"])
    _vs_oracle32(f"{name} fp32 variant {variant} broadcast", pre,
                 pre.solve(c["targets"][:8], np.zeros(pre.nq), dtype="f32", variant=variant), c["q"][:8],
                 c["converged"][:8], c["iters"][:8])


# ---------------------------------------------------------------- ragged batches
@pytest.mark.parametrize("name,dtype,variant,which", [
    ("nx_scaled", "f32", PACKED, 1), ("nx_scaled", "f32", PAIR, 1), ("nx_scaled", "f64", PAIR, 1),
    ("nx_scaled", "f64", PAIR, 0), ("offset_wrist", "f64", AUTO, 1), ("offset_wrist", "f64", AUTO, 0)])
def test_ragged_batches_bit_equal(family, cases, name, dtype, variant, which):
    """A problem's answer does not depend on the batch size or its place in the
    batch: B = 1, 31, 33, 65, 130 (cases tiled) against the B = 24 call."""
    s = family(name)[which]
    c = cases[name]
    ref = s.solve(c["targets"], c["q0"], dtype=dtype, variant=variant)
    for B in (1, 31, 33, 65, 130):
        idx = np.arange(B) % 24
        sol = s.solve(c["targets"][idx], c["q0"][idx], dtype=dtype, variant=variant)
        assert np.array_equal(sol.converged, ref.converged[idx]) and np.array_equal(sol.iters, ref.iters[idx]), B
        assert np.array_equal(sol.q, ref.q[idx]) and np.array_equal(sol.err, ref.err[idx]), B


# ---------------------------------------------------------------- damped, multistart
@pytest.mark.parametrize("name", ["offset_wrist", "nx_scaled", "hand_general"])
def test_damped(family, cases, name):
    jit, pre = family(name)
    c = cases[name]
    a, b = jit.solve(c["targets"], c["q0"], lam=1e-6), pre.solve(c["targets"], c["q0"], lam=1e-6)
    print(f"{name} damped jit vs prebuilt: {_same(a, b):.2e}")
    if name in rf.DAMPED:  # the oracle's loop with the step J^T (J J^T + lam I)^-1 e
        for tag, sol in (("prebuilt", b), ("jit", a)):
            _vs_oracle64(f"{name} damped {tag}", sol, c["q_damped"], c["converged_damped"], c["iters_damped"], c["err_damped"])


def test_multistart_generic_qr_path(family, cases):
    """test_gpu_generic.py's test_multistart_generic_path on kSpecGeneric."""
    c = cases["offset_wrist"]
    for s in family("offset_wrist"):
        seeds = np.stack([np.zeros(s.nq), c["q_star"]])
        ms = s.solve_multistart(c["targets"][:8], seeds)
        for t in range(8):
            per = s.solve(np.repeat(c["targets"][t:t + 1], 2, axis=0), seeds)
            b = ms.best_seed[t]
            assert ms.converged[t] == per.converged[b] and np.array_equal(ms.q[t], per.q[b])


# ---------------------------------------------------------------- FK and frame kinematics
@pytest.mark.parametrize("name", rf.NAMES)
def test_fk_and_local_jacobian(family, cases, name):
    _, s = family(name)
    c = cases[name]
    hands = s.fk(c["fk_q"])
    r = s.frame_kinematics(c["fk_q"], None, rf=1, outputs=("placement", "J"))
    d = [float(np.abs(x - y).max()) for x, y in ((hands, c["fk_hands"]), (r["placement"], c["fk_hands"]), (r["J"], c["fk_J"]))]
    print(f"{name}: fk {d[0]:.1e}, frame placement {d[1]:.1e}, LOCAL J {d[2]:.1e}")
    assert max(d) <= 1e-12


@pytest.mark.parametrize("rf_", [0, 1, 2])
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-12), ("f32", 2e-4)])
@pytest.mark.parametrize("name", rf.THREE_FRAME)
def test_frame_kinematics_three_frames(family, cases, name, dtype, tol, rf_):
    """ikg_frame_kinematics_batch's spec dispatch, with test_gpu_control.py's bounds."""
    _, s = family(name)
    c = cases[name]
    r = s.frame_kinematics(c["fk_q"], c["fk_v"], rf=rf_, outputs=KEYS, dtype=dtype)
    for k in KEYS:
        ref = c[f"{k}_rf{rf_}"]
        bound = tol * max(1.0, np.abs(ref).max() / 10)
        e = float(np.abs(r[k] - ref).max())
        print(f"{name} {dtype} rf {rf_} {k}: {e:.2e} (bound {bound:.2e})")
        assert e <= bound, k
    if dtype == "f64":  # columns outside a hand's support are exact zeros
        m = s.model
        for h in range(2):
            off = [j for j in range(m.nq) if j not in {m.root_q, *m.arm_q[h]}]
            assert np.all(r["J"][:, 6 * h:6 * h + 6, off] == 0) and np.all(r["dJ"][:, 6 * h:6 * h + 6, off] == 0)


# ---------------------------------------------------------------- the collision continuation with kSpecGeneric
def test_collision_term_generic_qr(cases):
    """check_collision on offset_wrist (kSpecGeneric): flags and update counts
    of the prebuilt and the specialised path equal the host emulator's with the
    same ikg_collision_desc, converged q within 1e-9; successes are collision-free."""
    from ikgrasp.solver import IKSolver
    m = rf.load_model(rf.COLLISION)
    scene = rf.collision_scene(m)
    c = cases[rf.COLLISION]
    q, conv, it, _ = host_emu.solve(m, c["targets"], c["q0"], scene=scene)
    _, conv0, it0, _ = host_emu.solve(m, c["targets"], c["q0"])
    assert ((conv != conv0) | (it != it0)).sum() >= 3 and conv.sum() >= 3
    for which, spec in (("prebuilt", False), ("jit", "auto")):
        s = IKSolver(m, device=0, scene=scene, specialize=spec)
        if spec:
            s.specialize("f64")
        sol = s.solve(c["targets"], c["q0"], check_collision=True)
        assert s.is_specialized("f64") == bool(spec)
        same = np.array_equal(sol.converged, conv) and np.array_equal(sol.iters, it)
        dq = float(np.abs(sol.q[conv] - q[conv]).max()) if same else float("nan")
        print(f"collision term {which}: flags/counts {'equal' if same else 'DIFFER'}, |dq| {dq:.2e}, successes {int(conv.sum())}")
        assert same, (sol.converged.tolist(), sol.iters.tolist(), it.tolist())
        assert dq <= 1e-9
        assert not s.collision(sol.q[conv], c["targets"][conv]).any()
        s.close()
