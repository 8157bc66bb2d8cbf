"""The robot family (tests/robot_family.py) on the CPU: which tables and
specialisation the model compiler gives each member, the committed fixtures'
case-set conditions, the compiled tables' FK / LOCAL Jacobian against the
raw-axis oracle, and the kernel arithmetic (host emulator, fp64 and fp32, each
member's own specialisation and the forced 6x6 QR path) against the oracle's
IK fixtures (tests/golden/family_cases.npz, oracle/generic_oracle.py).

Tolerances (test_generic_model.py / test_gpu_generic.py): fp64 identical
flags and update counts, converged q within 1e-9; fp32 identical flags,
counts within +-2, hand SE(3) distance to the fp64 fixture <= 1e-4.  Every
check prints its largest error."""
import ctypes as C

import numpy as np
import pytest

import emu as host_emu
import robot_family as rf
from helpers import fk_tables, hands_from_tables, se3_err
from ikgrasp import _lib

GENERIC = 99  # ikg_params.variant the emulator reads as "force the generic path"


@pytest.fixture(scope="module")
def cases():
    return rf.load_cases()


@pytest.fixture(scope="module")
def models():
    return {n: rf.load_model(n) for n in rf.NAMES}


@pytest.fixture(scope="module")
def emu():
    return host_emu.load_or_skip()


def model_info(emu, model):
    out = np.empty(8, np.int32)
    desc = _lib.model_desc(model)
    assert emu.ikg_emu_model_info(C.byref(desc), out.ctypes.data) == 0
    return dict(zip(rf.INFO, out.tolist()))


@pytest.mark.parametrize("name", rf.NAMES)
def test_model_tables(emu, models, name):
    """The last column of the family table: spec, wrist, hand_axis, rot_mask,
    zmask, pattern, n_passive, nq as build_kmodel / choose_spec see the member."""
    got, m = model_info(emu, models[name]), models[name]
    print(name, got)
    assert got == rf.MEMBERS[name]["expect"]
    if name in ("nx_scaled", "nx_extra_zero"):
        assert got["spec"] == rf.SPEC_NEXTAGE and (got["zmask"] & rf.ZERO_NEXTAGE) == rf.ZERO_NEXTAGE
    if name == "nx_extra_zero":
        assert got["zmask"] != rf.ZERO_NEXTAGE  # a JIT ZMASK the prebuilt kernels do not have
    if name == "nx_zbreak":
        assert got["pattern"] == rf.PATTERN_NEXTAGE and (got["zmask"] & rf.ZERO_NEXTAGE) != rf.ZERO_NEXTAGE
    if name == "hand_cross":  # Spec::fold_hand = axis(7) == axis(6)
        assert got["hand_axis"] in (0, 1) and got["hand_axis"] != (got["pattern"] >> 12) & 3
    if name == "mixed_axes":
        assert got["pattern"] & 3 == 1 and m.arm_q[1][0] < m.arm_q[0][0] and m.nq == _lib.IKG_MAX_NQ
        p = m.passive_q
        assert p[0] < m.arm_q[1][0] and any(m.arm_q[1][5] < j < m.arm_q[0][0] for j in p) and p[-1] > m.arm_q[0][5]
        assert not np.allclose(m.axis_frames(), np.eye(3))  # negative / unaligned axes were conjugated


def test_wrist_test_threshold(emu):
    """The two sides of parallel_or_zero's 1e-14: arm joint 5 1e-13 m off joint
    4's axis is no spherical wrist (wrist_edge); 1e-17 m is one."""
    from ikgrasp.model import DualArmModel, parse_urdf
    for eps, spec, wrist in ((1e-13, rf.SPEC_GENERIC, 0), (1e-17, rf.SPEC_GENERIC_WRIST, 1)):
        row = rf.wrist_edge_variant(eps)
        m = DualArmModel.from_trees(parse_urdf(rf.robot_urdf("wrist_edge", row)), parse_urdf(rf.cube_urdf("wrist_edge")))
        got = model_info(emu, m)
        assert (got["spec"], got["wrist"]) == (spec, wrist), (eps, got)


@pytest.mark.parametrize("name", rf.NAMES)
def test_case_set_conditions(cases, name):
    c = cases[name]
    n_conv, n_unconv, n_lim, n_dropped = (int(x) for x in c["counts"])
    print(name, dict(converged=n_conv, unconverged=n_unconv, on_limit=n_lim, dropped=n_dropped,
                     lstsq_dq=float(c["lstsq_dq"])))
    assert len(c["targets"]) == 24 and n_conv == int(c["converged"].sum()) and n_unconv == 24 - n_conv
    assert n_conv >= 12 and n_unconv >= 2 and n_lim >= 4 and n_dropped <= 4
    assert float(c["lstsq_dq"]) <= 1e-10
    assert np.all(c["q0"][:8] == 0) and len(c["fk_q"]) == 16
    m = rf.load_model(name)
    if m.passive_q:  # two warm cases start the passive joints outside their limits
        p = m.passive_q
        out = ((c["q0"][:, p] > m.upper[p]) | (c["q0"][:, p] < m.lower[p])).all(axis=1)
        assert out.sum() == 2 and out[-2:].all()
    act = [m.root_q] + m.arm_q.reshape(-1).tolist()
    on = ((c["q"][:, act] == m.lower[act]) | (c["q"][:, act] == m.upper[act])).any(axis=1)
    assert int(on.sum()) == n_lim


@pytest.mark.parametrize("name", rf.NAMES)
def test_generator_text_equals_committed_files(name):
    """The robot's text comes from the table alone and is equal character by
    character.  The cube's hook frames are computed (FK at q*, rpy): equal text
    apart from the numbers' last digits, which follow the host's maths library
    (numbers within 1e-14)."""
    import re
    robot, cube = rf.paths(name)
    with open(robot) as f:
        assert f.read() == rf.robot_urdf(name)
    with open(cube) as f:
        a, b = f.read(), rf.cube_urdf(name)
    num = r'(?<=[" ])-?\d+\.\d+(?:e-?\d+)?(?=[" ])'
    assert re.sub(num, "#", a) == re.sub(num, "#", b)
    na, nb = (np.array([float(x) for x in re.findall(num, t)]) for t in (a, b))
    assert len(na) == 1 + 12 and np.abs(na - nb).max() <= 1e-14  # the XML version and two (xyz, rpy)


@pytest.mark.parametrize("name", rf.NAMES)
def test_compiled_fk_and_jacobian_match_raw_axis_oracle(models, cases, name):
    m, c = models[name], cases[name]
    worst = [0.0, 0.0]
    for q, hands, J in zip(c["fk_q"], c["fk_hands"], c["fk_J"]):
        worst[0] = max(worst[0], float(np.abs(hands_from_tables(m, q) - hands).max()))
        oMi = fk_tables(m, q)
        Jt = np.zeros((12, m.nq))
        for h in range(2):
            Rf, pf = hands[h, :9].reshape(3, 3), hands[h, 9:]
            for j in [m.root_q] + list(m.arm_q[h]):
                a = oMi[j][0][:, int(m.axis[j])]
                Jt[6 * h:6 * h + 3, j] = Rf.T @ np.cross(a, pf - oMi[j][1])
                Jt[6 * h + 3:6 * h + 6, j] = Rf.T @ a
        worst[1] = max(worst[1], float(np.abs(Jt - J).max()))
    print(f"{name}: compiled tables vs raw-axis oracle: FK {worst[0]:.1e}, LOCAL J {worst[1]:.1e}")
    assert worst[0] <= 1e-14 and worst[1] <= 1e-14


def _check64(name, leg, got, q_ref, conv_ref, it_ref):
    q, conv, it, _ = got
    ok = conv_ref.astype(bool)
    same = np.array_equal(conv, ok) and np.array_equal(it, it_ref)
    dq = float(np.abs(q[ok] - q_ref[ok]).max()) if same else float("nan")
    print(f"{name} {leg}: flags/counts {'equal' if same else 'DIFFER'}, converged |dq| max {dq:.2e}")
    assert same, (conv.tolist(), it.tolist())
    assert dq <= 1e-9


@pytest.mark.parametrize("variant", [0, GENERIC])
@pytest.mark.parametrize("name", rf.NAMES)
def test_emulated_kernel_fp64(emu, models, cases, name, variant):
    m, c = models[name], cases[name]
    _check64(name, f"fp64 variant {variant}", host_emu.solve(m, c["targets"], c["q0"], variant=variant),
             c["q"], c["converged"], c["iters"])
    # the broadcast seed (short trig series with the exact fallback) on the cold cases
    _check64(name, f"fp64 variant {variant} broadcast q0", host_emu.solve(m, c["targets"][:8], np.zeros(m.nq), variant=variant),
             c["q"][:8], c["converged"][:8], c["iters"][:8])


@pytest.mark.parametrize("variant", [0, GENERIC])
@pytest.mark.parametrize("name", rf.DAMPED)
def test_emulated_kernel_damped(emu, models, cases, name, variant):
    m, c = models[name], cases[name]
    _check64(name, f"fp64 damped variant {variant}", host_emu.solve(m, c["targets"], c["q0"], variant=variant, lam=1e-6),
             c["q_damped"], c["converged_damped"], c["iters_damped"])


@pytest.mark.parametrize("variant", [0, GENERIC])
@pytest.mark.parametrize("name", rf.NAMES)
def test_emulated_kernel_fp32(emu, models, cases, name, variant):
    m, c = models[name], cases[name]
    q, conv, it, _ = host_emu.solve(m, c["targets"], c["q0"], dtype=1, variant=variant)
    ok = c["converged"].astype(bool)
    dit = int(np.abs(it[ok].astype(int) - c["iters"][ok]).max())
    h32 = np.array([hands_from_tables(m, x.astype(np.float64)) for x in q[ok]])
    h64 = np.array([hands_from_tables(m, x) for x in c["q"][ok]])
    e = max(float(se3_err(h32[:, h, :9].reshape(-1, 3, 3), h32[:, h, 9:], h64[:, h, :9].reshape(-1, 3, 3),
                          h64[:, h, 9:]).max()) for h in range(2))
    print(f"{name} fp32 variant {variant}: flags {'equal' if np.array_equal(conv, ok) else 'DIFFER'}, "
          f"count difference max {dit}, hand SE(3) distance max {e:.2e}")
    assert np.array_equal(conv, ok)
    assert dit <= 2 and e <= 1e-4


def test_collision_term_changes_answers(emu, models, cases):
    """offset_wrist's scene (URDF primitives, table, cube): the table stands so
    that the collision term changes the flag or the update count of at least 3
    of the 24 cases in the emulator's answer (the GPU leg compares with it)."""
    m, c = models[rf.COLLISION], cases[rf.COLLISION]
    scene = rf.collision_scene(m)
    _, conv0, it0, _ = host_emu.solve(m, c["targets"], c["q0"])
    _, conv1, it1, _ = host_emu.solve(m, c["targets"], c["q0"], scene=scene)
    changed = (conv0 != conv1) | (it0 != it1)
    print(f"collision term: {int(changed.sum())} of 24 cases change; successes {int(conv1.sum())} (without: {int(conv0.sum())})")
    assert changed.sum() >= 3 and conv1.sum() >= 3
