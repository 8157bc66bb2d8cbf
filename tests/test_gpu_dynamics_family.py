"""The dynamics and controller kernels on every robot-family tree (GPU leg;
models, fixture and the emulator's leg: tests/dynamics_family_cases.py,
tests/golden/dynamics_family_cases.npz, tests/test_dynamics_family.py).

csrc/ikg_dynamics.hip gives a state G lanes (16 for nq <= 16, else 32).  What
the lanes add to the emulator's arithmetic -- the parent fetch across a group,
idle lanes, the ancestor bit tests up to bit 31, the zero-filled LDS tile of M
with its mirrored writes, tile_store's two branches, the stores under r < 12
-- is judged here on nq = 13, 15, 16 (G = 16) and 17, 32, 32 (G = 32), in
fp64 and fp32, against the bounds the emulator meets on the CPU.

Bounds: fp64 M / nle / g 1e-12 x max(1, max|fixture|); fp32 tol32_<out>;
controller outputs tol_<out> of the model against the 50-digit evaluation.
Exact: M equals its transpose, M is 0.0 wherever neither joint is an ancestor
of the other (a stale or misplaced tile entry a tolerance would hide), qdd is 0
on passive joints, tau on the joints of the default zero_tau_mask."""
import ctypes as C

import numpy as np
import pytest

import dynamics_family_cases as fc
from helpers import report

pytestmark = pytest.mark.gpu

DYN, CTL = fc.DYN, fc.CTL
G16, G32 = ("nx_scaled", "nx_extra_zero"), ("mixed_17", "mixed_axes", "mixed_deep")
SHAPES = [(n, B) for n in G16 for B in (1, 3, 4, 5, 9)] + [(n, B) for n in G32 for B in (1, 2, 3, 5)]


@pytest.fixture(scope="module")
def cases():
    return fc.load_cases()


@pytest.fixture(scope="module")
def family(cases):
    """name -> (solver, the 8-state answers every other call is compared with):
    made on first use, kept for the module, closed at its end."""
    from ikgrasp.solver import IKSolver
    made = {}

    def get(name):
        if name not in made:
            model, bi = fc.models()[name]
            s = IKSolver(model, device=0, specialize=False)
            s.set_inertia(bi)
            c = cases[name]
            made[name] = (s, {"f64": s.dynamics(c["q"], c["v"], outputs=DYN), "f32": s.dynamics(c["q"], c["v"], outputs=DYN, dtype="f32"),
                              "ctl": s.control_torques(c["q"], c["v"], c["q_des"], c["v_des"])})
        return made[name]

    yield get
    for s, _ in made.values():
        s.close()


GUARD, TAIL = -7.25, 64


def _raw_dynamics(s, q, v, dtype, skip=0):
    """ikg_dynamics_batch with device pointers into buffers filled with GUARD,
    M starting `skip` elements into its buffer (the solver's own calls hand the
    kernel fresh or recycled memory, where a store that never happened can
    leave the right number behind).  Returns the outputs; the guards before M
    and behind every output must be untouched, and no output element may be
    left a guard."""
    import torch
    from ikgrasp import _lib
    from ikgrasp.solver import _dtype
    tt = torch.float64 if dtype == "f64" else torch.float32
    B, nq = q.shape
    dq, dv = (torch.tensor(x, device="cuda", dtype=tt) for x in (q, v))
    size = {"M": B * nq * nq, "nle": B * nq, "g": B * nq}
    buf = {k: torch.full((skip * (k == "M") + n + TAIL,), GUARD, device="cuda", dtype=tt) for k, n in size.items()}
    assert all(b.data_ptr() % 16 == 0 for b in buf.values())
    out = _lib.DynamicsOut(buf["M"].data_ptr() + skip * buf["M"].element_size(), buf["nle"].data_ptr(), buf["g"].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert s.lib.ikg_dynamics_batch(s._h, 0, _dtype(dtype)[0], dq.data_ptr(), dv.data_ptr(), B, C.byref(out), stream, 0) == 0
    torch.cuda.synchronize()
    res = {}
    for k, n in size.items():
        got, lo = buf[k].cpu().numpy(), skip * (k == "M")
        assert np.all(got[:lo] == GUARD) and np.all(got[lo + n:] == GUARD), k
        assert not np.any(got[lo:lo + n] == GUARD), k
        res[k] = got[lo:lo + n].reshape((B, nq, nq) if k == "M" else (B, nq))
    return res


def _raw_control(s, q, v, q_des, v_des):
    """ikg_control_torque_batch with device pointers into GUARD-filled buffers, as _raw_dynamics."""
    import torch
    from ikgrasp import _lib
    B, nq = q.shape
    ins = [torch.tensor(x, device="cuda", dtype=torch.float64) for x in (q, v, q_des, v_des)]
    size = {"tau": B * nq, "qdd": B * nq, "xdd": B * 12, "Lambda": B * 72, "fc": B * 12}
    buf = {k: torch.full((n + TAIL,), GUARD, device="cuda", dtype=torch.float64) for k, n in size.items()}
    out = _lib.ControlOut(*[buf[k].data_ptr() for k in CTL])
    prm = _lib.control_params()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert s.lib.ikg_control_torque_batch(s._h, 0, *[x.data_ptr() for x in ins], B, C.byref(prm), C.byref(out), stream, 0) == 0
    torch.cuda.synchronize()
    res = {}
    for k, n in size.items():
        got = buf[k].cpu().numpy()
        assert np.all(got[n:] == GUARD) and not np.any(got[:n] == GUARD), k
        res[k] = got[:n].reshape((B, 2, 36) if k == "Lambda" else (B, -1))
    return res


def _zero_tau_joints():
    from ikgrasp import _lib
    mask = _lib.control_params().zero_tau_mask  # the default of every call here (control.py:404: joints 1 and 2)
    return [j for j in range(32) if (mask >> j) & 1]


# ---------------------------------------------------------------- a, b: against the fixture
@pytest.mark.parametrize("name", fc.NAMES)
def test_dynamics_match_fixture(cases, family, name):
    model = fc.models()[name][0]
    _, base = family(name)
    c, row = cases[name], {}
    for k in DYN:
        ref = c[k]
        row[k] = {"fp64": np.abs(base["f64"][k] - ref).max() / max(1.0, np.abs(ref).max()),
                  "fp32": np.abs(base["f32"][k].astype(np.float64) - ref).max() / np.abs(ref).max(),
                  "bound32": cases[""]["tol32_" + k]}
    report(f"dynamics_family_gpu_{name}", row)
    for k in DYN:
        assert row[k]["fp64"] <= 1e-12, k
        assert row[k]["fp32"] <= row[k]["bound32"], k
    rel = fc.related(model.parents)
    for dt in ("f64", "f32"):
        M = base[dt]["M"]
        assert np.array_equal(M, M.transpose(0, 2, 1)), dt
        assert np.all(M[:, ~rel] == 0.0) and np.all(M[:, rel] != 0.0), dt


@pytest.mark.parametrize("name", fc.NAMES)
def test_control_torques_within_measured_bounds(cases, family, name):
    model = fc.models()[name][0]
    ctl, c = family(name)[1]["ctl"], cases[name]
    row = {k: {"err": np.abs(ctl[k] - c[k + "_mp"]).max() / np.abs(c[k + "_mp"]).max(), "restatement": c["err_f64_" + k],
               "bound": c["tol_" + k]} for k in CTL}
    report(f"control_family_gpu_{name}", row)
    for k in CTL:
        assert row[k]["err"] <= row[k]["bound"], k
    assert np.all(ctl["qdd"][:, model.passive_q] == 0)
    zt = _zero_tau_joints()
    assert zt == [1, 2] and np.all(ctl["tau"][:, zt] == 0)
    assert np.all(np.delete(ctl["tau"], zt, axis=1) != 0)


# ---------------------------------------------------------------- c: batch shapes
@pytest.mark.parametrize("name,B", SHAPES)
def test_batch_shapes(cases, family, name, B):
    """Every row of a B-state call (states i % 8) equals the 8-state call's row
    bit for bit: tile tails, more than one workgroup, and both branches of
    tile_store (16-byte stores need dst and n * sizeof(T) to be multiples of
    16; a workgroup holds 4 states at G = 16 and 2 at G = 32, one state of M is
    nq^2 elements, and every workgroup's dst is a multiple of a full tile):

      nq = 13 (169 elements a state), fp64 and fp32: a full tile (4 states) is a
        multiple of 16 bytes, 1 or 3 states are not.  B = 1, 3: fallback;
        B = 4: 16-byte; B = 5, 9: 16-byte workgroups and a one-state fallback tail.
      nq = 16, nq = 32: a state is a multiple of 16 bytes: 16-byte at every B.
      nq = 17 (289 elements), fp64: a full tile (2 states) is 16 x 289 bytes, one
        state is not.  B = 1: fallback; B = 2: 16-byte; B = 3, 5: 16-byte
        workgroups and a one-state fallback tail.
      nq = 17, fp32: a full tile is 2312 bytes = 16 x 144 + 8, so full tiles take
        the fallback too, and every second workgroup's dst sits 8 bytes off a
        16-byte boundary (B = 3, 5).  No row takes the 16-byte branch."""
    s, base = family(name)
    c = cases[name]
    idx = np.arange(B) % fc.N_STATES
    for dt in ("f64", "f32"):
        r = _raw_dynamics(s, c["q"][idx], c["v"][idx], dt)
        for k in DYN:
            assert r[k].shape[0] == B and np.array_equal(r[k], base[dt][k][idx]), (dt, k)
    r = _raw_control(s, c["q"][idx], c["v"][idx], c["q_des"][idx], c["v_des"][idx])
    for k in CTL:
        assert r[k].shape[0] == B and np.array_equal(r[k], base["ctl"][k][idx]), k


# ---------------------------------------------------------------- d: output subsets, v = None
@pytest.mark.parametrize("name", ["mixed_axes", "nx_extra_zero"])
def test_output_subsets_and_zero_velocity(cases, family, name):
    """Each output alone equals the all-outputs call bit for bit (nle or g
    alone is the launch without M: no tile, no dynamic LDS), in both types;
    without v, nle is g."""
    s, base = family(name)
    c = cases[name]
    for dt in ("f64", "f32"):
        for k in DYN:
            assert np.array_equal(s.dynamics(c["q"], c["v"], outputs=(k,), dtype=dt)[k], base[dt][k]), (dt, k)
        r0 = s.dynamics(c["q"], None, outputs=("nle", "g"), dtype=dt)
        assert np.array_equal(r0["nle"], r0["g"]) and np.array_equal(r0["g"], base[dt]["g"]), dt
        assert not np.array_equal(base[dt]["nle"], base[dt]["g"])
    for k in CTL:
        r = s.control_torques(c["q"], c["v"], c["q_des"], c["v_des"], outputs=(k,))
        assert np.array_equal(r[k], base["ctl"][k]), k


# ---------------------------------------------------------------- e: a misaligned caller buffer
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["nx_scaled", "mixed_axes"])
def test_misaligned_M_buffer(cases, family, name, dtype):
    """M one element into a device buffer (8 bytes off a 16-byte boundary in
    fp64, 4 in fp32), B = 5: every workgroup's dst is misaligned, so full
    tiles whose byte count is a multiple of 16 take tile_store's fallback.  The
    answer equals the aligned call's bit for bit and the guards on both sides
    of M are untouched."""
    s, base = family(name)
    c = cases[name]
    idx = np.arange(5) % fc.N_STATES
    aligned = _raw_dynamics(s, c["q"][idx], c["v"][idx], dtype)
    shifted = _raw_dynamics(s, c["q"][idx], c["v"][idx], dtype, skip=1)
    for k in DYN:
        assert np.array_equal(shifted[k], aligned[k]) and np.array_equal(shifted[k], base[dtype][k][idx]), k


# ---------------------------------------------------------------- f: host and device routes
def test_host_and_device_calls_agree(cases, family):
    import torch
    s, base = family("mixed_17")
    c = cases["mixed_17"]
    for dt, tt in (("f64", torch.float64), ("f32", torch.float32)):
        dev = lambda k: torch.tensor(c[k], device="cuda", dtype=tt)
        rd = s.dynamics(dev("q"), dev("v"), outputs=DYN)
        torch.cuda.synchronize()
        for k in DYN:
            assert np.array_equal(rd[k].cpu().numpy(), base[dt][k]), (dt, k)
    dev = lambda k: torch.tensor(c[k], device="cuda", dtype=torch.float64)
    rc = s.control_torques(dev("q"), dev("v"), dev("q_des"), dev("v_des"))
    torch.cuda.synchronize()
    for k in CTL:
        assert np.array_equal(rc[k].cpu().numpy(), base["ctl"][k]), k
