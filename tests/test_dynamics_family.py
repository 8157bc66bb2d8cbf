"""The dynamics and controller kernels' arithmetic on every robot-family tree
(CPU leg; the GPU leg is tests/test_gpu_dynamics_family.py): the models of
tests/dynamics_family_cases.py, the fixture
tests/golden/dynamics_family_cases.npz (make_dynamics_family_golden.py) and
the host emulation (ikg_emu_dynamics, ikg_emu_control_torque) against it.

The emulator has no lanes, so what it shows is that the fixture's bounds are
reachable by the kernels' own arithmetic on these trees and that the host
tables (anc, levels, ref, grav) are right -- where nothing depends on a GPU.
Bounds: fp64 M / nle / g 1e-12 x max(1, max|fixture|); fp32 tol32_<out>
(8 x the float32 oracle's largest error on any model); controller outputs
tol_<out> (20 x the float64 restatement's error against 50 digits)."""
import numpy as np
import pytest

import dynamics_family_cases as fc
import dynamics_oracle as do
import emu as host_emu
import robot_family as rf
from helpers import report
from test_dynamics import _emu_control

DYN, CTL = fc.DYN, fc.CTL
NQ = {"nx_scaled": 13, "nx_extra_zero": 16, "mixed_axes": 32, "mixed_17": 17, "mixed_deep": 32}  # the others: 15
CHAIN = {"mixed_axes": 11, "mixed_deep": 17}  # longest chain; the others: root + arm = 7


@pytest.fixture(scope="module")
def cases():
    return fc.load_cases()


@pytest.fixture(scope="module")
def emu():
    return host_emu.load()


# ---------------------------------------------------------------- the models
def test_family_covers_both_lane_groups_and_their_edges():
    ms = fc.models()
    assert set(ms) == set(rf.NAMES) | {"mixed_17", "mixed_deep"}
    for name, (m, bi) in ms.items():
        assert m.nq == bi.nq == NQ.get(name, 15), name
        assert fc.longest_chain(m.parents) == CHAIN.get(name, 7), name
    assert sorted(m.nq for m, _ in ms.values()) == [13] + [15] * 6 + [16, 17, 32, 32]
    assert {fc.group_lanes(m.nq) for m, _ in ms.values()} == {16, 32}
    assert "mixed_17" not in rf.MEMBERS and "mixed_deep" not in rf.MEMBERS


def test_mixed_17_is_mixed_axes_without_two_chains():
    m, base = fc.models()["mixed_17"][0], fc.models()["mixed_axes"][0]
    keep = [j for j, n in enumerate(base.joint_names) if not n.startswith(("AA_JOINT", "M_JOINT"))]
    assert m.joint_names == [base.joint_names[j] for j in keep] and m.nq == 1 + 6 + 6 + 4
    new_of = {old: k for k, old in enumerate(keep)}
    assert m.parents == [new_of.get(base.parents[j], -1) for j in keep]
    for name in ("R", "t", "axis", "lower", "upper", "Q"):
        assert np.array_equal(getattr(m, name), getattr(base, name)[keep]), name
    for name in ("hand_R", "hand_t", "hook_R", "hook_t"):
        assert np.array_equal(getattr(m, name), getattr(base, name)), name
    assert np.array_equal(m.arm_q, [[new_of[j] for j in row] for row in base.arm_q])
    assert fc.first_arm(m) == 1 and len(m.passive_q) == 4  # the right arm first, T_JOINT after the arms


def test_mixed_deep_hangs_the_chain_below_the_first_arm():
    base = fc.models()["mixed_axes"][0]
    m, perm = fc.mixed_deep_model()
    chain = fc.deep_chain(base)
    assert chain == list(range(1, 11)) and fc.first_arm(base) == 1
    assert perm == [0] + list(range(11, 32)) + chain
    new_of = {old: k for k, old in enumerate(perm)}
    assert m.joint_names == [base.joint_names[o] for o in perm]
    assert m.passive_q == sorted(new_of[j] for j in base.passive_q)
    assert np.array_equal(m.arm_q, [[new_of[j] for j in row] for row in base.arm_q]) and m.root_q == 0
    tip = int(m.arm_q[1][-1])
    assert tip == 6 and m.parents[22:] == [tip] + list(range(22, 31))  # parents in the upper half of the group
    for k, o in enumerate(perm):
        if o != chain[0]:
            assert m.parents[k] == (new_of[base.parents[o]] if base.parents[o] >= 0 else -1)
        assert np.array_equal(m.R[k], base.R[o]) and np.array_equal(m.t[k], base.t[o]) and m.axis[k] == base.axis[o]
    d = fc.depths(m.parents)
    assert max(d) == d[31] == 1 + 6 + 10


def test_chain_helper_rejects_what_it_cannot_move():
    base = fc.models()["mixed_axes"][0]
    chain = fc.deep_chain(base)
    for bad in (chain[:5], chain[::-1], [chain[0], chain[2]], [int(base.arm_q[0][0])]):
        with pytest.raises(ValueError):
            do.hanging_passive_model(base, chain=bad, below=base.arm_q[1][-1])
    with pytest.raises(ValueError):
        do.hanging_passive_model(base, chain=chain, below=chain[3])


# ---------------------------------------------------------------- the fixture, independent of the product
@pytest.mark.parametrize("name", fc.NAMES)
def test_fixture_properties(cases, name):
    model, bi = fc.models()[name]
    c = cases[name]
    for k, x in zip(("q", "v", "q_des", "v_des"), fc.states(name, model)):
        assert np.array_equal(c[k], x), k
    assert c["M"].shape == (fc.N_STATES, model.nq, model.nq)
    assert np.all(c["q"] >= model.lower) and np.all(c["q"] <= model.upper) and np.abs(c["q"]).max() <= 2.0
    assert np.array_equal(c["M"], c["M"].transpose(0, 2, 1))
    np.linalg.cholesky(c["M"])  # raises LinAlgError unless positive definite
    rel = fc.related(model.parents)
    assert np.all(c["M"][:, ~rel] == 0.0) and np.all(c["M"][:, rel] != 0.0)
    assert rel.sum() < model.nq ** 2  # two arms: some pair is unrelated
    t = do.Tree(do.F64, model, bi)
    for i in (0, fc.N_STATES - 1):
        assert np.array_equal(c["g"][i], do.nle(t, c["q"][i], np.zeros(model.nq)))
        assert np.array_equal(c["M"][i], do.crba(t, c["q"][i]))
        assert np.array_equal(c["nle"][i], do.nle(t, c["q"][i], c["v"][i]))
    assert np.abs(c["nle"] - c["g"]).max() > 1e-3  # the velocities matter
    assert np.all(c["tau_mp"][:, [1, 2]] == 0) and np.all(c["qdd_mp"][:, model.passive_q] == 0)
    for k in CTL:
        assert c["tol_" + k] == 20.0 * c["err_f64_" + k] > 0, k
    for k in DYN:
        assert cases[""]["tol32_" + k] == 8.0 * max(cases[n]["fp32_err_" + k] for n in fc.NAMES), k


# ---------------------------------------------------------------- the kernels' arithmetic on the host
@pytest.mark.parametrize("name", fc.NAMES)
def test_emulated_dynamics_match_fixture(emu, cases, name):
    model, bi = fc.models()[name]
    c = cases[name]
    r64 = host_emu.dynamics(model, bi, c["q"], c["v"], 0)
    r32 = host_emu.dynamics(model, bi, c["q"], c["v"], 1)
    row = {}
    for k in DYN:
        ref = c[k]
        e64 = np.abs(r64[k] - ref).max() / max(1.0, np.abs(ref).max())
        e32 = np.abs(r32[k].astype(np.float64) - ref).max() / np.abs(ref).max()
        row[k] = {"fp64": e64, "fp32": e32, "bound32": cases[""]["tol32_" + k]}
    report(f"dynamics_family_emu_{name}", row)
    for k in DYN:
        assert row[k]["fp64"] <= 1e-12, k
        assert row[k]["fp32"] <= row[k]["bound32"], k
    rel = fc.related(model.parents)
    for r in (r64, r32):
        assert np.array_equal(r["M"], r["M"].transpose(0, 2, 1)) and np.all(r["M"][:, ~rel] == 0.0)


@pytest.mark.parametrize("name", fc.NAMES)
def test_emulated_control_solve_within_measured_bounds(emu, cases, name):
    model, bi = fc.models()[name]
    c = cases[name]
    r = _emu_control(model, bi, c, fc.N_STATES)
    row = {k: {"err": np.abs(r[k] - c[k + "_mp"]).max() / np.abs(c[k + "_mp"]).max(), "restatement": c["err_f64_" + k],
               "bound": c["tol_" + k]} for k in CTL}
    report(f"control_family_emu_{name}", row)
    for k in CTL:
        assert row[k]["err"] <= row[k]["bound"], k
    assert np.all(r["tau"][:, 1:3] == 0) and np.all(r["qdd"][:, model.passive_q] == 0)
