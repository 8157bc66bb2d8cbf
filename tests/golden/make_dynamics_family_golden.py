"""Writes tests/golden/dynamics_family_cases.npz from tests/dynamics_oracle.py
on the models of tests/dynamics_family_cases.py (the nine robots of
tests/golden/family plus mixed_17 and mixed_deep; seeded inertias).

    python tests/golden/make_dynamics_family_golden.py

The recipe of make_dynamics_golden.py, per model; 8 seeded states each
(dynamics_family_cases.states).  The robot family is this repository's own
test data: nothing here reads a file outside the repository.

Entries, `<model>.` in front of the per-model ones
  q, v, q_des, v_des [8,nq]
  M, nle, g                  float64 oracle (crba / nonLinearEffects / gravity)
  J, dJv, err, derr          the float64 oracle's kinematic terms (LOCAL_WORLD_ALIGNED): the inputs of the
                             emulator's controller entry
  tau, qdd, xdd, Lambda, fc  float64 numpy restatement of control.py:284-406
  *_mp                       the same outputs with everything (FK, dynamics, inverses) in 50-digit mpmath
                             arithmetic, rounded to float64: the truth.  No M_mp (8 KB a state at nq = 32).
  err_f64_<out>              the float64 restatement's largest error against *_mp over the 8 states,
                             relative to max|out_mp|
  tol_<out>                  the kernel's bound = 20 x err_f64_<out> of this model (factor and definition:
                             make_dynamics_golden.py).  The host emulation of the kernels' arithmetic meets
                             it on every model (tests/test_dynamics_family.py), so no bound is pooled.
  fp32_err_<M|nle|g>         the oracle in float32 against float64, relative to max|out|
  (in the file the scalars are one vector per model and kind -- err_f64 and tol in the order
  tau, qdd, xdd, Lambda, fc; fp32_err and the pooled tol32 in the order M, nle, g -- so that the file stays
  under the size of dynamics_cases.npz; dynamics_family_cases.load_cases returns them under the names above)
Pooled over the models
  tol32_<M|nle|g>            8 x the largest fp32_err_<out> of any model (the factor of
                             make_dynamics_golden.py).  Pooled because the maximum over 8 states of one
                             model is a noisy estimate of float32's error on it: per model it varies
                             several-fold between robots of the same size.
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

import dynamics_family_cases as fc  # noqa: E402
import dynamics_oracle as do  # noqa: E402

CTL, DYN = fc.CTL, fc.DYN


def _flat(r):
    return {k: do.to_f64(r[k]).reshape(-1) if k != "Lambda" else do.to_f64(r[k]).reshape(2, 36) for k in CTL}


def _one(args):
    name, i = args
    model, inert = fc.models()[name]
    q, v, qd, vd = (x[i] for x in fc.states(name, model))
    t64, tmp, t32 = (do.Tree(ar, model, inert) for ar in (do.F64, do.MP, do.F32))
    terms = do.task_space_terms(t64, q, v, qd, vd)
    out = {"J": terms[0], "dJv": terms[1], "err": terms[2], "derr": terms[3]}
    r64 = do.controllaw_terms(t64, q, v, qd, vd, terms=terms)
    out["M"], out["nle"], out["g"] = r64["M"], r64["nle"], do.gravity_torques(t64, q)
    out.update(_flat(r64))
    out.update({k + "_mp": x for k, x in _flat(do.controllaw_terms(tmp, q, v, qd, vd)).items()})
    out["M32"], out["nle32"], out["g32"] = (do.crba(t32, q).astype(np.float64), do.nle(t32, q, v).astype(np.float64),
                                            do.gravity_torques(t32, q).astype(np.float64))
    return out


def main():
    models = fc.models()
    jobs = [(name, i) for name in fc.NAMES for i in range(fc.N_STATES)]
    with Pool(min(16, os.cpu_count() or 1)) as p:
        res = dict(zip(jobs, p.map(_one, jobs)))
    d, per = {}, {}
    for name in fc.NAMES:
        model = models[name][0]
        c = dict(zip(("q", "v", "q_des", "v_des"), fc.states(name, model)))
        for k in res[(name, 0)]:
            c[k] = np.array([res[(name, i)][k] for i in range(fc.N_STATES)])
        for k in DYN:
            c[f"fp32_err_{k}"] = np.abs(c[k + "32"] - c[k]).max() / np.abs(c[k]).max()
            del c[k + "32"]
        for k in CTL:
            c[f"err_f64_{k}"] = np.abs(c[k] - c[k + "_mp"]).max() / np.abs(c[k + "_mp"]).max()
            c[f"tol_{k}"] = 20.0 * c[f"err_f64_{k}"]
        per[name] = c
    for k in DYN:
        d[f"tol32_{k}"] = 8.0 * max(per[n][f"fp32_err_{k}"] for n in fc.NAMES)
    print("float32 oracle vs float64, relative to max|out|      M         nle       g")
    for n in fc.NAMES:
        print(f"  {n:14s} nq {models[n][0].nq:2d}                        " + "  ".join(f"{per[n]['fp32_err_' + k]:.2e}" for k in DYN))
    print("  fp32 bounds (8 x the largest)                  " + "  ".join(f"{d['tol32_' + k]:.2e}" for k in DYN))
    print("float64 restatement vs 50 digits, relative to max|out| (bound)")
    print("  " + " " * 14 + "".join(f"  {k:21s}" for k in CTL))
    for n in fc.NAMES:
        print(f"  {n:14s}" + "".join(f"  {per[n]['err_f64_' + k]:.2e} ({per[n]['tol_' + k]:.2e})" for k in CTL))
    # the scalars go in as one vector per model and kind (an archive member costs more than it holds):
    # dynamics_family_cases.load_cases gives them back under the names above
    for kind, keys in fc.PACKED.items():
        if kind == "tol32":
            d[kind] = np.array([d.pop(f"{kind}_{k}") for k in keys])
            continue
        for n in fc.NAMES:
            per[n][kind] = np.array([per[n].pop(f"{kind}_{k}") for k in keys])
    for n in fc.NAMES:
        d.update({f"{n}.{k}": x for k, x in per[n].items()})
    path = os.path.join(HERE, "dynamics_family_cases.npz")
    np.savez_compressed(path, **d)
    print(f"wrote dynamics_family_cases.npz: {len(fc.NAMES)} models x {fc.N_STATES} states, {os.path.getsize(path)} bytes"
          f" (dynamics_cases.npz: {os.path.getsize(os.path.join(HERE, 'dynamics_cases.npz'))})")


if __name__ == "__main__":
    main()
