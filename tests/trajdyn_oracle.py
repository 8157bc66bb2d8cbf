"""CPU ORACLE -- test infrastructure only, never the product path.

The definitions of ikg_trajectory_dynamics_batch (include/ikgrasp.h) restated
on tests/dynamics_oracle.py (`rnea`, `Tree`: Pinocchio's body-local recursion,
which shares nothing with the kernel's world-frame one) and
tests/rollout_oracle.py's Horner, in any arithmetic `ar` (F64, or MP = 50
digits: the truth), and what tests/test_trajdyn.py (host emulator) and
tests/test_gpu_trajdyn.py share: the fixture tests/golden/trajdyn_cases.npz
(tests/golden/make_trajdyn_golden.py), its bars and the emulator's runner.

Per (curve, sample k, joint j), T = t_max - t_min:
  t_k = t_min + k T / (S - 1), t_{S-1} = t_max       (a float64 in every arithmetic: the input)
  q   = Bezier(P, t_min, t_max, mult)(t_k)
  v   = Bezier(n (P[i+1] - P[i]), ..., mult (1 / T))(t_k), n the degree;  a the same again from v
  tau = rnea(q, v, a),  g = rnea(q, 0, 0),  d = tau - g
  speed = |v| / vlim,  torque_use = |tau| / E,  static_use = |g| / E
  |g| >= E: static (counted, left out of torque_scale), else torque_scale = sqrt(|d| / (E - sign(d) g))
  an unlimited joint (limit >= NO_LIMIT) contributes 0
Per curve: the maximum of each ratio over (k, j) and its (sample, joint), the
lowest sample then the lowest joint among exact ties (numpy's argmax of the
[S, nq] array); torque_scale of a curve whose every entry is static is 0 at (-1, -1).

Bars (the convention of tests/golden/make_dynamics_golden.py): per case and
output the float64 oracle's largest deviation from the 50-digit answer relative
to max|out_mp| of the case; the kernel's bar is 20 x that.  For a ratio the
deviation is taken over the per-entry array [B, S, nq] whose maximum the
per-curve output is, exactly as for tau and g: a maximum moves by no more than
its entries do, and one scalar's deviation would measure one entry's luck.
"""
import os

import numpy as np

import dynamics_oracle as do
import rollout_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "trajdyn_cases.npz")
NO_LIMIT = 1e30
RATIOS = ("speed_scale", "torque_use", "static_use", "torque_scale")
ARGS = {"speed_scale": "arg_speed", "torque_use": "arg_torque_use", "static_use": "arg_static",
        "torque_scale": "arg_torque_scale"}
SAMPLE = ("tau", "g")
BAR_FACTOR = 20.0
ARG_GAP = 1e-6  # the generator's condition on every arg: the runner-up lies this far (relative) below the winner


def sample_times(t_min, t_max, S):
    """the entry's rule in float64 (trajcheck_time)"""
    t = [t_min + (k * (t_max - t_min)) / (S - 1) for k in range(S)]
    t[-1] = t_max
    return [float(x) for x in t]


def derivative(ar, curve):
    """Bezier.derivative(1) in arithmetic ar: points n (P[i+1] - P[i]), multiplier mult (1 / T)"""
    P, t_min, t_max, mult = curve
    with ro.keep_precision():
        P = do.arr(ar, P)
    n = ar.num(float(len(P) - 1))
    T = ar.num(t_max) - ar.num(t_min)
    m = mult if hasattr(mult, "_mpf_") else ar.num(mult)
    return (P[1:] - P[:-1]) * n, t_min, t_max, m * (ar.num(1.0) / T)


def _bezier(ar, curve, t):
    """rollout_oracle.bezier with control points and a multiplier already in the arithmetic"""
    with ro.keep_precision():
        return ro.bezier(ar, curve, t)


def curve_states(ar, points, t_min, t_max, mult, S):
    """-> q, v, a [S, nq] in arithmetic ar"""
    cq = (do.arr(ar, points), t_min, t_max, mult)
    cv = derivative(ar, cq)
    ca = derivative(ar, cv)
    rows = [[_bezier(ar, c, t) for c in (cq, cv, ca)] for t in sample_times(t_min, t_max, S)]
    return tuple(np.array([r[i] for r in rows], dtype=ar.dtype) for i in range(3))


def entries(ar, tree, points, t_min, t_max, mult, S, vlim, elim):
    """One curve -> dict of the per-entry arrays [S, nq] in arithmetic ar: tau,
    g, speed, torque_use, static_use, torque_scale (0 on static entries) and
    static (bool)."""
    q, v, a = curve_states(ar, points, t_min, t_max, mult, S)
    nq = tree.nq
    zero = np.zeros(nq)
    with ro.keep_precision():
        tau = np.array([do.rnea(tree, q[k], v[k], a[k]) for k in range(S)], dtype=ar.dtype)
        g = np.array([do.rnea(tree, q[k], zero, zero) for k in range(S)], dtype=ar.dtype)
    out = {"tau": tau, "g": g}
    for key in RATIOS:
        out[key] = do.zeros(ar, S, nq)
    out["static"] = np.zeros((S, nq), dtype=bool)
    out["d"] = tau - g
    for j in range(nq):
        vfree, efree = vlim[j] >= NO_LIMIT, elim[j] >= NO_LIMIT
        V, E = ar.num(float(vlim[j])), ar.num(float(elim[j]))
        for k in range(S):
            if not vfree:
                out["speed_scale"][k, j] = abs(v[k, j]) / V
            if efree:
                continue
            out["torque_use"][k, j] = abs(tau[k, j]) / E
            out["static_use"][k, j] = abs(g[k, j]) / E
            if abs(g[k, j]) >= E:
                out["static"][k, j] = True
                continue
            d = tau[k, j] - g[k, j]
            if d != 0:
                out["torque_scale"][k, j] = ar.sqrt(abs(d) / (E - g[k, j] if d > 0 else E + g[k, j]))
    return out


def fold(e):
    """One curve's per-entry arrays (float64) -> its per-curve outputs"""
    out = {"n_static": int(e["static"].sum())}
    nq = e["tau"].shape[1]
    for key in RATIOS:
        x = np.asarray(e[key], dtype=np.float64)
        if key == "torque_scale":
            if e["static"].all():
                out[key], out[ARGS[key]] = 0.0, (-1, -1)
                continue
            x = np.where(e["static"], -1.0, x)
        i = int(np.argmax(x))
        out[key], out[ARGS[key]] = float(x.reshape(-1)[i]), (i // nq, i % nq)
    return out


def arg_gap(e, key):
    """(winner - runner-up) / winner of a ratio's per-entry array; inf where the
    winner is 0 (every entry ties at exactly 0 in any arithmetic: the tie rule
    pins the arg) or where one entry takes part"""
    x = np.asarray(e[key], dtype=np.float64)
    if key == "torque_scale":
        x = x[~e["static"]]
    x = np.sort(x.reshape(-1))
    if len(x) < 2 or x[-1] == 0.0:
        return np.inf
    return float((x[-1] - x[-2]) / x[-1])


# ---------------------------------------------------------------- models
def model_of(name):
    """-> (DualArmModel, BodyInertias) of a fixture case's model"""
    if name == "nextage":
        from ikgrasp.model import load_nextage, load_nextage_inertia
        return load_nextage(), load_nextage_inertia()
    import dynamics_family_cases as dfc
    assert name == "mixed_17", name
    m = dfc.mixed_17_model()
    return m, do.seeded_inertias(m.nq, dfc.SEEDS["mixed_17"])


# ---------------------------------------------------------------- the fixture
_cache = {}


def cases():
    if "c" not in _cache:
        _cache["c"] = dict(np.load(FIXTURE))
    return _cache["c"]


def names():
    return [str(n) for n in cases()["names"]]


def case(name):
    """-> dict of the case's entries (its keys without the `<name>.` prefix)"""
    c = cases()
    d = {k[len(name) + 1:]: v for k, v in c.items() if k.startswith(name + ".")}
    d["name"] = name
    return d


def inputs(cs, idx=None):
    """-> (points [B,n,nq], t_min, t_max, mult, S, vlim, elim) of a case (or of its curves idx)"""
    pts = cs["points"] if idx is None else cs["points"][list(idx)]
    return (np.ascontiguousarray(pts), float(cs["range"][0]), float(cs["range"][1]), float(cs["range"][2]),
            int(cs["S"]), cs["vlim"], cs["elim"])


def bar(cs, key):
    """the kernel's absolute bar of output `key` in this case"""
    return BAR_FACTOR * float(cs["dev_" + key]) * float(cs["max_" + key])


def compare(cs, got, rows=None, verbose=False):
    """The answer `got` (curves `rows` of the case, default all) against the
    fixture's 50-digit answer under the case's bars; args and n_static exact."""
    rows = list(range(len(cs["points"]))) if rows is None else list(rows)
    fig = {}
    for key in SAMPLE + RATIOS:
        ref = cs[key + "_mp"][rows]
        fig[key] = float(np.abs(np.asarray(got[key]) - ref).max())
    if verbose:
        print(cs["name"], {k: f"{v:.3e}" for k, v in fig.items()}, "bars",
              {k: f"{bar(cs, k):.3e}" for k in SAMPLE + RATIOS})
    for key in SAMPLE + RATIOS:
        assert fig[key] <= bar(cs, key), (cs["name"], key, fig[key], bar(cs, key))
    for key in RATIOS:
        assert np.array_equal(np.asarray(got[ARGS[key]]), cs[ARGS[key]][rows]), (cs["name"], ARGS[key])
    assert np.array_equal(np.asarray(got["n_static"]), cs["n_static"][rows]), (cs["name"], "n_static")
    return fig


CURVE_KEYS = RATIOS + tuple(ARGS.values()) + ("n_static",)


def same(a, ja, b, jb, keys=CURVE_KEYS + SAMPLE):
    """Curve ja of answer a and curve jb of answer b are equal bit for bit"""
    for k in keys:
        assert np.array_equal(np.asarray(a[k][ja]), np.asarray(b[k][jb])), k


# ---------------------------------------------------------------- the emulator leg
def emu_runner(model, inertias, gravity=do.GRAVITY):
    """run(points, t_min, t_max, mult, S, vlim, elim, samples_per_wave=0) over
    ikg_emu_trajectory_dynamics -> dict of every output; rc != 0 raises ValueError"""
    import ctypes as C

    import emu as host_emu
    from ikgrasp import _lib
    lib = host_emu.load()
    md, idesc = _lib.model_desc(model), _lib.inertia_desc(inertias, gravity)
    nq = model.nq

    def run(points, t_min, t_max, mult, S, vlim, elim, samples_per_wave=0):
        pts = np.ascontiguousarray(points, dtype=np.float64)
        B, n = pts.shape[0], pts.shape[1]
        assert pts.shape[2] == nq
        res = {k: np.empty((B,) + tail, dtype=t) for k, t, tail in _lib.TRAJDYN_CURVE}
        res.update({k: np.empty((B, S, nq)) for k in _lib.TRAJDYN_SAMPLE})
        out = _lib.TrajDynOut(*[res[f[0]].ctypes.data for f in _lib.TRAJDYN_CURVE],
                              *[res[k].ctypes.data for k in _lib.TRAJDYN_SAMPLE])
        bset = _lib.BezierSet(pts.ctypes.data, n, float(t_min), float(t_max), float(mult))
        prm = _lib.TrajDynParams(int(S), int(samples_per_wave))
        for j in range(_lib.IKG_MAX_NQ):
            prm.velocity_limit[j] = float(vlim[j]) if j < nq else NO_LIMIT
            prm.effort_limit[j] = float(elim[j]) if j < nq else NO_LIMIT
        rc = lib.ikg_emu_trajectory_dynamics(C.byref(md), C.byref(idesc), C.byref(bset), B, C.byref(prm), C.byref(out))
        if rc != 0:
            raise ValueError(f"ikg_emu_trajectory_dynamics returned {rc}")
        return res

    return run
