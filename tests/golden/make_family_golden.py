"""Writes the fixtures of the robot family (tests/robot_family.py):

    python tests/golden/make_family_golden.py

  tests/golden/family/<member>.urdf, <member>_cube.urdf   the generator's text
  tests/golden/family_cases.npz                           keys "<member>.<entry>"

Every answer comes from oracle/generic_oracle.py (raw URDF axes, Rodrigues
rotations, np.linalg.pinv), which reads the URDF text itself.

Per member, 24 solve cases: 8 from q0 = 0 and 16 from q* + N(0, 0.1); targets
as make_golden.py's make_generic_cases (the cube between the hands at q*,
+-0.05 m, yaw +-0.25).  In two warm cases the passive joints start outside
their limits (members with passive joints).  A case whose oracle answer is not
robust to rounding is dropped and redrawn: it is solved again with the step by
np.linalg.lstsq instead of pinv, and dropped when the flag or the update
count moves, or a converged q moves by more than 1e-10.  Asserted here (and,
from the stored counts, in tests/test_robot_family.py): at most 4 draws
dropped, >= 12 cases converge, >= 2 do not, >= 4 final q have an active
joint on a limit.

Entries per member
  q_star [nq], center [3]
  targets [24,12], q0 [24,nq], q [24,nq], converged [24], iters [24], err [24,2]
  counts = (converged, unconverged, final q with an active joint on a limit, draws dropped);
  lstsq_dq (largest |q_pinv - q_lstsq| among the converged cases kept)
  fk_q, fk_v [16,nq]; fk_hands [16,2,12]; fk_J [16,12,nq] (LOCAL frame Jacobians, generic oracle)
  nx_scaled, offset_wrist, mixed_axes:  instead of fk_J, J_rf<r> and dJ_rf<r> [16,12,nq] for r = 0 WORLD,
      1 LOCAL, 2 LOCAL_WORLD_ALIGNED from robot_family.frame_kinematics, the spatial-algebra formulation
      of oracle/control_oracle.py on the raw axes (analytic dJ).  Checked here against (a) the generic
      oracle's LOCAL J (1e-14; J_rf1 stands for fk_J), (b) the central difference of J along v,
      h = 1e-6, to test_control.py's bound, and (c) tests/dynamics_oracle.py's frame_terms on the
      compiled model (LOCAL_WORLD_ALIGNED J, velocity, dJ v; 1e-12).  The placement is fk_hands, the
      frame velocity J v and dJv = dJ v with fk_v (identities asserted here to 1e-13): these are left
      out of the file and filled in by robot_family.load_cases.
  nx_scaled, offset_wrist:  q_damped, converged_damped, iters_damped, err_damped: the same loop with
      the step J^T (J J^T + lam I)^-1 e, lam = 1e-6 (generic_oracle.damped_step)
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "motion-planning-and-control-for-dual-manipulator-robot_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import robot_family as rf  # noqa: E402
from oracle import generic_oracle as go  # noqa: E402

N_COLD, N_WARM, N_FK, MAX_DROPS = 8, 16, 16, 4
LAM = 1e-6
_CACHE = {}


def _model(name):
    if name not in _CACHE:
        _CACHE[name] = (rf.chain_model(name), go.cube_hooks(rf.cube_urdf(name)))
    return _CACHE[name]


def _solve(args):
    name, tg, q0, step = args
    cm, hooks = _model(name)
    fn = {"pinv": None, "lstsq": go.lstsq_step, "damped": go.damped_step(LAM)}[step]
    q, ok, it, e = go.computeqgrasppose(cm, hooks, q0, tg[:9].reshape(3, 3), tg[9:], step=fn)
    return q, ok, it, e


def _draw(name, rng, cm, qs, center, warm, outside):
    """One (target, q0) draw."""
    yaw = rng.uniform(-0.25, 0.25)
    c, s = np.cos(yaw), np.sin(yaw)
    tg = np.concatenate([np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).reshape(9), center + rng.uniform(-0.05, 0.05, 3)])
    q0 = np.zeros(cm.nq)
    if warm:
        q0 = qs + rng.normal(scale=0.1, size=cm.nq)
        if outside:  # the passive joints start outside their limits
            for k, j in enumerate(_passive(name, cm)):
                q0[j] = cm.upper[j] + 0.3 if k % 2 == 0 else cm.lower[j] - 0.2
    return tg, q0


def _active(name, cm):
    m = rf.MEMBERS[name]
    names = [m["root"]["name"]] + [f"{p}{k}" for p in m["arm_names"] for k in range(6)]
    return [cm.names.index(n) for n in names]


def _passive(name, cm):
    act = set(_active(name, cm))
    return [j for j in range(cm.nq) if j not in act]


def solve_cases(name, pool):
    cm, _ = _model(name)
    qs, center = rf.q_star(name, cm), rf.grasp_center(name, cm)
    rng = np.random.default_rng(1000 + rf.NAMES.index(name))
    n = N_COLD + N_WARM
    slots = [(i >= N_COLD, i >= n - 2) for i in range(n)]
    draws = [_draw(name, rng, cm, qs, center, *s) for s in slots]
    res, dropped, worst = [None] * n, 0, 0.0
    todo = list(range(n))
    while todo:
        a = pool.map(_solve, [(name, *draws[i], "pinv") for i in todo])
        b = pool.map(_solve, [(name, *draws[i], "lstsq") for i in todo])
        again = []
        for i, ra, rb in zip(todo, a, b):
            dq = float(np.abs(ra[0] - rb[0]).max())
            if ra[1] != rb[1] or ra[2] != rb[2] or (ra[1] and dq > 1e-10):
                dropped += 1
                assert dropped <= MAX_DROPS, f"{name}: more than {MAX_DROPS} draws are not robust to rounding"
                draws[i] = _draw(name, rng, cm, qs, center, *slots[i])
                again.append(i)
            else:
                res[i] = ra
                if ra[1]:
                    worst = max(worst, dq)
        todo = again
    q = np.array([r[0] for r in res])
    conv = np.array([r[1] for r in res])
    act = _active(name, cm)
    on_limit = ((q[:, act] == cm.lower[act]) | (q[:, act] == cm.upper[act])).any(axis=1)
    d = dict(q_star=qs, center=center, targets=np.array([t for t, _ in draws]), q0=np.array([s for _, s in draws]),
             q=q, converged=conv, iters=np.array([r[2] for r in res], dtype=np.int32), err=np.array([r[3] for r in res]),
             counts=np.array([int(conv.sum()), int((~conv).sum()), int(on_limit.sum()), dropped]), lstsq_dq=worst)
    n_conv, n_unconv, n_lim, _ = d["counts"]
    print(f"{name:14s} nq {cm.nq:2d}: converged {n_conv:2d}/24 (cold {int(conv[:N_COLD].sum())}), on a limit "
          f"{n_lim:2d}, dropped {dropped}, pinv vs lstsq |dq| {worst:.1e}, iters {d['iters'].tolist()}")
    assert n_conv >= 12 and n_unconv >= 2 and n_lim >= 4, name
    if name in rf.DAMPED:
        r = pool.map(_solve, [(name, *draws[i], "damped") for i in range(n)])
        d.update(q_damped=np.array([x[0] for x in r]), converged_damped=np.array([x[1] for x in r]),
                 iters_damped=np.array([x[2] for x in r], dtype=np.int32), err_damped=np.array([x[3] for x in r]))
        print(f"{'':14s} damped: converged {int(d['converged_damped'].sum())}, iters moved in "
              f"{int((d['iters_damped'] != d['iters']).sum())} cases")
    return d


def fk_cases(name):
    import dynamics_oracle as do
    from ikgrasp.model import DualArmModel, parse_urdf
    cm, _ = _model(name)
    rng = np.random.default_rng(2000 + rf.NAMES.index(name))
    q = rng.uniform(cm.lower, cm.upper, size=(N_FK, cm.nq))
    v = rng.normal(0.0, 0.7, size=(N_FK, cm.nq))
    hands, Jl = [], []
    for x in q:
        o = cm.fk(x)
        hands.append([np.concatenate([cm.frame(o, h)[0].reshape(9), cm.frame(o, h)[1]]) for h in ("LARM_EFF", "RARM_EFF")])
        Jl.append(np.vstack([cm.frame_jacobian_local(x, h, o) for h in ("LARM_EFF", "RARM_EFF")]))
    d = dict(fk_q=q, fk_v=v, fk_hands=np.array(hands), fk_J=np.array(Jl))
    if name not in rf.THREE_FRAME:
        return d
    model = DualArmModel.from_trees(parse_urdf(rf.robot_urdf(name), rf.base_placement(name)), parse_urdf(rf.cube_urdf(name)))
    tree = do.Tree(do.F64, model, do.seeded_inertias(model.nq, 0))
    h = 1e-6
    worst = dict(J_local=0.0, fd=0.0, tree=0.0)
    for r in (0, 1, 2):
        rs = [rf.frame_kinematics(cm, q[i], v[i], r) for i in range(N_FK)]
        for k in ("J", "dJ"):  # placement = fk_hands, velocity = J v, dJv = dJ v: robot_family.load_cases
            d[f"{k}_rf{r}"] = np.array([x[k] for x in rs])
        assert np.abs(np.array([x["placement"] for x in rs]) - d["fk_hands"]).max() <= 1e-14
        for i in range(N_FK):
            fd = (rf.frame_kinematics(cm, q[i] + h * v[i], v[i], r)["J"] - rf.frame_kinematics(cm, q[i] - h * v[i], v[i], r)["J"]) / (2 * h)
            e = np.abs(fd - rs[i]["dJ"]).max() / max(1.0, np.abs(v[i]).max())
            worst["fd"] = max(worst["fd"], e)
            assert e <= 5e-8, (name, r, i, e)  # tests/test_control.py: dJ = d/dt J(q + t v)
            np.testing.assert_allclose((rs[i]["J"] @ v[i]).reshape(2, 6), rs[i]["velocity"], atol=1e-13)
            np.testing.assert_allclose(rs[i]["dJ"] @ v[i], rs[i]["dJv"], atol=1e-13)
    worst["J_local"] = float(np.abs(d["J_rf1"] - d["fk_J"]).max())
    assert worst["J_local"] <= 1e-14
    for i in range(N_FK):
        for hnd, ((R, p), vel, Jt, dJv) in enumerate(do.frame_terms(tree, q[i], v[i])):
            Jo, dJo = d["J_rf2"][i, 6 * hnd:6 * hnd + 6], d["dJ_rf2"][i, 6 * hnd:6 * hnd + 6]
            for a, b in ((vel, Jo @ v[i]), (Jt, Jo), (dJv, dJo @ v[i])):
                worst["tree"] = max(worst["tree"], float(np.abs(a - b).max()))
    assert worst["tree"] <= 1e-12, (name, worst)
    del d["fk_J"]  # = J_rf1 to 1e-14 (checked above)
    print(f"{'':14s} three-frame terms: LOCAL J vs generic oracle {worst['J_local']:.1e}, dJ vs central difference "
          f"{worst['fd']:.1e} (bound 5e-8), LWA vel/J/dJv vs dynamics_oracle on the compiled model {worst['tree']:.1e}")
    return d


def main(only=None):
    os.makedirs(rf.FAMILY_DIR, exist_ok=True)
    out = {}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for name in rf.NAMES:
            if only and name not in only:
                continue
            robot, cube = rf.paths(name)
            with open(robot, "w") as f:
                f.write(rf.robot_urdf(name))
            with open(cube, "w") as f:
                f.write(rf.cube_urdf(name))
            d = solve_cases(name, pool)
            d.update(fk_cases(name))
            out.update({f"{name}.{k}": x for k, x in d.items()})
    if only:
        return
    path = os.path.join(HERE, "family_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; dynamics_cases.npz:",
          os.path.getsize(os.path.join(HERE, "dynamics_cases.npz")))


if __name__ == "__main__":
    main(sys.argv[1:])
