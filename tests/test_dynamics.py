"""Controller dynamics and torques on the CPU (control.py:284-406): the body
inertia compile, the oracle (tests/dynamics_oracle.py) against the definitions
of the quantities -- none of which shares code with the algorithms under test
(Pinocchio is not importable here) -- the host emulation of the kernels'
arithmetic against the fixtures (tests/golden/dynamics_cases.npz, whose tol_*
entries are the measured bounds), and the C-ABI argument checks.  The
emulation on every robot-family tree: tests/test_dynamics_family.py."""
import ctypes as C
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import dynamics_oracle as do
import emu as host_emu
from conftest import GOLDEN, ROOT
from helpers import fk_tables
from ikgrasp import _lib
from ikgrasp.model import (BodyInertias, DualArmModel, load_nextage, load_nextage_inertia, parse_urdf, rpy_to_matrix,
                           sym6_matrix)

URDF = os.path.join(GOLDEN, "NextageaOpen.urdf")
CTL = ("tau", "qdd", "xdd", "Lambda", "fc")
G = np.array(do.GRAVITY)


@pytest.fixture(scope="module")
def dc():
    return dict(np.load(os.path.join(GOLDEN, "dynamics_cases.npz")))


@pytest.fixture(scope="module")
def nextage():
    m, bi = load_nextage(), load_nextage_inertia()
    return m, bi, do.Tree(do.F64, m, bi)


@pytest.fixture(scope="module")
def tilted():
    m = DualArmModel.from_urdf(os.path.join(GOLDEN, "tilted_dualarm.urdf"), os.path.join(GOLDEN, "tilted_cube.urdf"))
    return m, do.seeded_inertias(m.nq, 1)


@pytest.fixture(scope="module")
def emu():
    return host_emu.load()


# ---------------------------------------------------------------- inertia compile
def test_shipped_inertia_is_the_urdf_compile():
    a, b = load_nextage_inertia(), BodyInertias.from_urdf(URDF)
    assert np.array_equal(a.mass, b.mass) and np.array_equal(a.com, b.com) and np.array_equal(a.inertia, b.inertia)
    a.validate()
    rt = BodyInertias.from_json(a.to_json())
    assert np.array_equal(rt.inertia, a.inertia) and np.array_equal(rt.com, a.com)


def test_body_masses_sum_to_the_movable_links():
    tree = parse_urdf(URDF)
    root = ET.parse(URDF).getroot()
    total = sum(float(l.find("inertial/mass").get("value")) for l in root.findall("link") if l.find("inertial") is not None)
    fixed = sum(m for name, (m, _, _, _) in tree.inertials.items() if tree.frames[name].parent < 0)
    assert fixed > 0  # the base and waist links hang off the universe
    assert load_nextage_inertia().mass.sum() == pytest.approx(total - fixed, rel=1e-15)


THREE_LINK = """<robot name="t">
 <link name="base"><inertial><mass value="9"/><origin xyz="1 2 3"/><inertia ixx="1" iyy="1" izz="1" ixy="0" ixz="0" iyz="0"/></inertial></link>
 <link name="arm"><inertial><mass value="2.0"/><origin xyz="0.1 -0.2 0.3" rpy="0.3 -0.4 0.5"/>
   <inertia ixx="0.02" ixy="0.001" ixz="-0.002" iyy="0.03" iyz="0.0015" izz="0.025"/></inertial></link>
 <link name="tool"><inertial><mass value="0.7"/><origin xyz="-0.05 0.02 0.04" rpy="-0.7 0.2 1.1"/>
   <inertia ixx="0.004" ixy="0.0002" ixz="0.0001" iyy="0.005" iyz="-0.0003" izz="0.003"/></inertial></link>
 <joint name="j" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0.5 0 1" rpy="0.1 0.2 0.3"/>
   <axis xyz="0 -1 0"/><limit lower="-1" upper="1"/></joint>
 <joint name="f" type="fixed"><parent link="arm"/><child link="tool"/><origin xyz="0.2 0.1 -0.3" rpy="0.6 -0.5 0.4"/></joint>
</robot>"""


def test_fixed_child_transport_and_negative_axis():
    """One revolute joint (-Y axis), a fixed child with an offset and rotated
    inertial origins: the merged body equals the parallel-axis result worked
    out here, in the canonical frame (Q = diag(-1, -1, 1): a half turn about Z)."""
    bi = BodyInertias.from_urdf(THREE_LINK)
    assert bi.nq == 1
    Q = np.diag([-1.0, -1.0, 1.0])
    I1 = np.array([[0.02, 0.001, -0.002], [0.001, 0.03, 0.0015], [-0.002, 0.0015, 0.025]])
    I2 = np.array([[0.004, 0.0002, 0.0001], [0.0002, 0.005, -0.0003], [0.0001, -0.0003, 0.003]])
    R1 = rpy_to_matrix(0.3, -0.4, 0.5)
    Rf, tf = rpy_to_matrix(0.6, -0.5, 0.4), np.array([0.2, 0.1, -0.3])
    R2 = Rf @ rpy_to_matrix(-0.7, 0.2, 1.1)
    c1, c2 = np.array([0.1, -0.2, 0.3]), tf + Rf @ np.array([-0.05, 0.02, 0.04])
    m1, m2 = 2.0, 0.7
    m = m1 + m2
    c = (m1 * c1 + m2 * c2) / m
    par = lambda mass, d: mass * (d @ d * np.eye(3) - np.outer(d, d))
    I = R1 @ I1 @ R1.T + par(m1, c1 - c) + R2 @ I2 @ R2.T + par(m2, c2 - c)
    assert bi.mass[0] == pytest.approx(m, rel=1e-15)
    np.testing.assert_allclose(bi.com[0], Q.T @ c, rtol=0, atol=1e-15)
    np.testing.assert_allclose(sym6_matrix(bi.inertia[0]), Q.T @ I @ Q, rtol=0, atol=1e-15)


def test_validate_rejects_unphysical_bodies():
    ok = do.seeded_inertias(3, 0)
    for change in ("mass", "indefinite", "triangle"):
        b = BodyInertias(ok.mass.copy(), ok.com.copy(), ok.inertia.copy())
        if change == "mass":
            b.mass[1] = -1.0
        elif change == "indefinite":
            b.inertia[1] = [1.0, 0, 0, -0.5, 0, 1.0]
        else:
            b.inertia[1] = [1.0, 0, 0, 1.0, 0, 3.0]
        with pytest.raises(ValueError):
            b.validate()


# ---------------------------------------------------------------- the oracle against definitions
def _link_points(tree_raw, model, q):
    """World (mass, centre, R, I_com) of every movable link from the kinematic
    tree's link frames and the raw <inertial> entries (no merged inertias)."""
    oMi = fk_tables(model, q)
    out = []
    for name, (m, xyz, Ro, I) in tree_raw.inertials.items():
        f = tree_raw.frames[name]
        if f.parent < 0:
            continue
        Rj, tj = oMi[f.parent]
        out.append((m, tj + Rj @ (f.t + f.R @ xyz), Rj @ f.R @ Ro, I, f.parent))
    return out


def _potential(tree_raw, model, q):
    return -sum(m * G @ c for m, c, _, _, _ in _link_points(tree_raw, model, q))


def test_gravity_is_the_gradient_of_the_potential(dc, nextage):
    model, _, t = nextage
    raw = parse_urdf(URDF, (np.eye(3), np.array([0.0, 0.0, 0.85])))
    h = 1e-6
    for i in range(20):
        q = dc["q"][4 * i]
        g = do.gravity_torques(t, q)
        fd = np.zeros(model.nq)
        for j in range(model.nq):
            e = np.zeros(model.nq)
            e[j] = h
            fd[j] = (_potential(raw, model, q + e) - _potential(raw, model, q - e)) / (2 * h)
        np.testing.assert_allclose(g, fd, rtol=0, atol=5e-8 * np.abs(g).max())
        assert abs(g[model.root_q]) <= 1e-12  # vertical chest axis
        np.testing.assert_allclose(dc["g"][4 * i], g, rtol=0, atol=1e-13)


def _support(model, j):
    out = []
    while j >= 0:
        out.append(j)
        j = model.parents[j]
    return out


def test_M_equals_its_definition(dc, nextage):
    """M = sum over links of m Jc^T Jc + Jw^T R I R^T Jw with geometric link
    Jacobians (axis x (c - o)) built from FK alone."""
    model, _, t = nextage
    raw = parse_urdf(URDF, (np.eye(3), np.array([0.0, 0.0, 0.85])))
    for i in range(0, 96, 5):
        q = dc["q"][i]
        oMi = fk_tables(model, q)
        M = np.zeros((model.nq, model.nq))
        for m, c, R, I, j in _link_points(raw, model, q):
            Jc, Jw = np.zeros((3, model.nq)), np.zeros((3, model.nq))
            for k in _support(model, j):
                a = oMi[k][0][:, int(model.axis[k])]
                Jc[:, k], Jw[:, k] = np.cross(a, c - oMi[k][1]), a
            M += m * Jc.T @ Jc + Jw.T @ R @ I @ R.T @ Jw
        Mo = do.crba(t, q)
        np.testing.assert_allclose(Mo, M, rtol=0, atol=1e-12 * np.abs(M).max())
        assert np.array_equal(Mo, Mo.T)
        assert np.linalg.eigvalsh(Mo)[0] > 0
        np.testing.assert_allclose(dc["M"][i], Mo, rtol=0, atol=1e-14)


def test_nle_is_the_christoffel_form_and_M_is_rnea_columns(dc, nextage):
    model, _, t = nextage
    n, h = model.nq, 1e-6
    for i in (3, 41, 88):
        q, v = dc["q"][i], dc["v"][i]
        dM = np.zeros((n, n, n))  # dM[k] = dM/dq_k
        for k in range(n):
            e = np.zeros(n)
            e[k] = h
            dM[k] = (do.crba(t, q + e) - do.crba(t, q - e)) / (2 * h)
        cv = np.einsum("kij,j,k->i", dM, v, v) - 0.5 * np.einsum("ijk,j,k->i", dM, v, v)
        c = do.nle(t, q, v) - do.gravity_torques(t, q)
        np.testing.assert_allclose(c, cv, rtol=0, atol=5e-7 * np.abs(c).max())
        M = do.crba(t, q)
        z = np.zeros(n)
        base = do.rnea(t, q, z, z)
        for k in range(n):
            e = np.zeros(n)
            e[k] = 1.0
            np.testing.assert_allclose(M[:, k], do.rnea(t, q, z, e) - base, rtol=0, atol=1e-12)


def test_oracle_kinematic_terms_equal_control_oracle(dc, nextage):
    """The oracle's own point-velocity kinematic terms (used in 50 digits)
    against oracle/control_oracle.py's spatial-algebra ones."""
    from oracle import control_oracle as co
    _, _, t = nextage
    for i in (0, 50, 90):
        a = do.task_space_terms(t, dc["q"][i], dc["v"][i], dc["q_des"][i], dc["v_des"][i])
        b = co.task_space_terms(dc["q"][i], dc["v"][i], dc["q_des"][i], dc["v_des"][i])
        for x, y in zip(a, b):
            np.testing.assert_allclose(x, y, rtol=0, atol=1e-12 * max(1.0, np.abs(y).max()))


def test_controller_restatement_properties(dc, nextage):
    model, _, t = nextage
    J, qdd, xdd, dJv = dc["J"], dc["qdd"], dc["xdd"], dc["dJv"]
    head = model.passive_q
    for i in range(96):
        H = J[i].T @ J[i] + 1e-6 * np.eye(model.nq)
        d = J[i].T @ (xdd[i] - dJv[i])
        # the normal equations, to the residual a backward-stable float64 solve leaves
        assert np.abs(H @ qdd[i] - d).max() <= 64 * np.finfo(float).eps * (np.abs(H) @ np.abs(qdd[i]) + np.abs(d)).max()
    assert np.all(dc["tau"][:, 1] == 0) and np.all(dc["tau"][:, 2] == 0)
    assert np.all(qdd[:, head] == 0) and np.all(dc["qdd_mp"][:, head] == 0)
    # on the trajectory, without force terms: xdd = 0, qdd = -(J^T J + r I)^-1 J^T dJv, tau = M qdd + nle
    q, v = dc["q"][7], dc["v"][7]
    r = do.controllaw_terms(t, q, v, q, v, Kf=0.0, Kt=0.0, fc_bias=np.zeros(12), zero_tau=())
    assert np.all(r["xdd"] == 0)
    Jt, dJvt, _, _ = do.task_space_terms(t, q, v, q, v)
    want = -np.linalg.solve(Jt.T @ Jt + 1e-6 * np.eye(model.nq), Jt.T @ dJvt)
    np.testing.assert_allclose(r["qdd"], want, rtol=0, atol=1e-9 * np.abs(want).max())
    np.testing.assert_allclose(r["tau"], r["M"] @ r["qdd"] + r["nle"], rtol=0, atol=1e-12 * np.abs(r["tau"]).max())


# ---------------------------------------------------------------- the kernels' arithmetic on the host
@pytest.mark.parametrize("which", ["nextage", "tilted"])
def test_emulated_dynamics_match_fixtures(emu, dc, nextage, tilted, which):
    if which == "nextage":
        model, bi, pre, q, v = nextage[0], nextage[1], "", dc["q"], dc["v"]
    else:
        model, bi, pre, q, v = tilted[0], tilted[1], "tilted_", dc["tilted_q"], dc["tilted_v"]
    r64 = host_emu.dynamics(model, bi, q, v, 0)
    r32 = host_emu.dynamics(model, bi, q, v, 1)
    for k in ("M", "nle", "g"):
        ref = dc[pre + k]
        e64 = np.abs(r64[k] - ref).max() / np.abs(ref).max()
        e32 = np.abs(r32[k].astype(np.float64) - ref).max() / np.abs(ref).max()
        print(f"{which} {k}: fp64 {e64:.2e} (bound 1e-12), fp32 {e32:.2e} (bound {float(dc[pre + 'tol32_' + k]):.2e})")
        assert e64 <= 1e-12, k
        assert e32 <= float(dc[pre + "tol32_" + k]), k
    assert np.array_equal(r64["M"], r64["M"].transpose(0, 2, 1))


def _emu_control(model, bi, dc, n, **gains):
    return host_emu.control_torque(model, bi, *(dc[k][:n] for k in host_emu.CONTROL_IN), **gains)


def test_emulated_control_solve_within_measured_bounds(emu, dc, nextage):
    model, bi, _ = nextage
    r = _emu_control(model, bi, dc, 96)
    for k in CTL:
        ref = dc[k + "_mp"]
        err = np.abs(r[k] - ref).max() / np.abs(ref).max()
        print(f"{k}: {err:.3e} of max|.| (float64 restatement {float(dc['err_f64_' + k]):.3e}, bound {float(dc['tol_' + k]):.3e})")
        assert err <= float(dc["tol_" + k]), k
    assert np.all(r["tau"][:, 1:3] == 0) and np.all(r["qdd"][:, model.passive_q] == 0)


def test_emulated_control_solve_honours_gains(emu, dc, nextage):
    model, bi, _ = nextage
    g = dict(zip(("Kp", "Kv", "Kf", "Kt", "lambda_reg", "qp_reg"), dc["gains_alt"]))
    r = _emu_control(model, bi, dc, 8, fc_bias=dc["fc_bias_alt"], **g)
    base = _emu_control(model, bi, dc, 8)
    for k in CTL:
        ref = dc[k + "_alt_mp"]
        assert np.abs(r[k] - ref).max() <= float(dc["tol_" + k]) * np.abs(ref).max(), k
    assert np.abs(r["tau"] - base["tau"]).max() > 1.0


# ---------------------------------------------------------------- C-ABI
@pytest.fixture()
def handle():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ikg_model_create(C.byref(_lib.model_desc(load_nextage())), C.byref(h)) == 0
    yield lib, h
    lib.ikg_model_destroy(h)


def test_entries_reject_bad_arguments(handle):
    lib, h = handle
    msg = lambda: lib.ikg_last_error().decode()
    buf = np.zeros(15)
    p = buf.ctypes.data
    dout, cout, prm = _lib.DynamicsOut(), _lib.ControlOut(), _lib.control_params()
    HOST = _lib.IKG_FLAG_HOST_POINTERS
    # no inertia attached yet
    assert lib.ikg_dynamics_batch(h, 0, 0, p, None, 1, C.byref(dout), None, HOST) == -1 and "inertia" in msg()
    assert lib.ikg_control_torque_batch(h, 0, p, p, p, p, 1, C.byref(prm), C.byref(cout), None, HOST) == -1
    assert "inertia" in msg()
    idesc = _lib.inertia_desc(load_nextage_inertia())
    assert lib.ikg_model_set_inertia(h, C.byref(idesc)) == 0
    assert lib.ikg_model_set_inertia(h, None) == -1 and lib.ikg_model_set_inertia(None, C.byref(idesc)) == -1
    assert lib.ikg_dynamics_batch(None, 0, 0, p, None, 1, C.byref(dout), None, HOST) == -1
    assert lib.ikg_dynamics_batch(h, 0, 0, None, None, 1, C.byref(dout), None, HOST) == -1 and "q is required" in msg()
    assert lib.ikg_dynamics_batch(h, 0, 0, p, None, 1, None, None, HOST) == -1 and "out is NULL" in msg()
    assert lib.ikg_dynamics_batch(h, 0, 0, p, None, -1, C.byref(dout), None, HOST) == -1 and "B must be" in msg()
    assert lib.ikg_dynamics_batch(h, 0, 7, p, None, 1, C.byref(dout), None, HOST) == -1 and "dtype" in msg()
    assert lib.ikg_control_torque_batch(h, 0, None, p, p, p, 1, C.byref(prm), C.byref(cout), None, HOST) == -1
    assert lib.ikg_control_torque_batch(h, 0, p, p, None, p, 1, C.byref(prm), C.byref(cout), None, HOST) == -1
    assert "q_des" in msg()
    assert lib.ikg_control_torque_batch(h, 0, p, p, p, p, -2, C.byref(prm), C.byref(cout), None, HOST) == -1
    assert lib.ikg_control_torque_batch(h, 0, p, p, p, p, 1, None, C.byref(cout), None, HOST) == -1
    assert lib.ikg_control_torque_batch(h, 0, p, p, p, p, 1, C.byref(prm), None, None, HOST) == -1
    bad = buf.copy()
    bad[4] = np.nan
    assert lib.ikg_dynamics_batch(h, 0, 0, bad.ctypes.data, None, 1, C.byref(dout), None, HOST) == -1
    assert "not finite" in msg()
    assert lib.ikg_dynamics_batch(h, 0, 0, p, bad.ctypes.data, 1, C.byref(dout), None, HOST) == -1
    assert lib.ikg_control_torque_batch(h, 0, bad.ctypes.data, p, p, p, 1, C.byref(prm), C.byref(cout), None, HOST) == -1
    assert "not finite" in msg()
    assert lib.ikg_control_torque_batch(h, 0, p, p, p, bad.ctypes.data, 1, C.byref(prm), C.byref(cout), None, HOST) == -1


def test_set_inertia_rejects_unphysical_bodies(handle):
    lib, h = handle
    for change in ("mass", "indefinite", "triangle", "nan"):
        d = _lib.inertia_desc(load_nextage_inertia())
        if change == "mass":
            d.mass[3] = -0.1
        elif change == "indefinite":
            d.inertia[3][:] = [1.0, 0.0, 0.0, -0.5, 0.0, 1.0]
        elif change == "triangle":
            d.inertia[3][:] = [1.0, 0.0, 0.0, 1.0, 0.0, 3.0]
        else:
            d.com[3][1] = float("nan")
        assert lib.ikg_model_set_inertia(h, C.byref(d)) == -1, change
        assert "body 3" in lib.ikg_last_error().decode()


def test_control_params_default_are_the_references():
    p = _lib.control_params()
    assert (p.Kp, p.Kf, p.lambda_reg, p.qp_reg) == (7000.0, 30.0, 1e-6, 1e-6)
    assert p.Kv == 2 * np.sqrt(7000.0) and p.Kt == 2 * np.sqrt(30.0)
    assert list(p.fc_bias) == [0.0, -200.0] + [0.0] * 10 and p.zero_tau_mask == 0b110


def _binding():
    """examples/ikgrasp_binding.py with the package's config / tools standing in for the reference's."""
    import importlib
    import sys
    from ikgrasp import config, tools
    saved = {k: sys.modules.get(k) for k in ("config", "tools")}
    sys.modules["config"], sys.modules["tools"] = config, tools
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        return importlib.import_module("ikgrasp_binding")
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_ctypes_structures_match_the_header(tmp_path):
    """Sizes and field offsets of the new structures, in ikgrasp/_lib.py and in
    the reference-side binding, from a C probe (tests/abi_probe_dynamics.c)
    compiled against include/ikgrasp.h."""
    exe = str(tmp_path / "abi_probe_dynamics")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "abi_probe_dynamics.c")], check=True)
    rows = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    b = _binding()
    for structs in ({"ikg_inertia_desc": _lib.InertiaDesc, "ikg_dynamics_out": _lib.DynamicsOut,
                     "ikg_control_params": _lib.ControlParams, "ikg_control_out": _lib.ControlOut},
                    {"ikg_inertia_desc": b.IDesc, "ikg_dynamics_out": b.DynOut,
                     "ikg_control_params": b.CtlParams, "ikg_control_out": b.CtlOut}):
        seen = set()
        for name, field, off, size in rows:
            cls = structs[name]
            if field == "sizeof":
                assert C.sizeof(cls) == int(size), name
            else:
                f = getattr(cls, field)
                assert (f.offset, f.size) == (int(off), int(size)), (name, field)
            seen.add((name, field))
        for name, cls in structs.items():
            for field, _ in cls._fields_:
                assert (name, field) in seen, (name, field)
