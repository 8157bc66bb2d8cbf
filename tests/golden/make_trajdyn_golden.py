"""Writes tests/golden/trajdyn_cases.npz from tests/trajdyn_oracle.py.

    python tests/golden/make_trajdyn_golden.py            regenerate
    python tests/golden/make_trajdyn_golden.py --check    regenerate and compare every array bit for bit

The cases of ikg_trajectory_dynamics_batch (each S <= 33, the smallest shapes
that can still go wrong).  The reference's recorded trajectory is data read
from tests/golden/rollout_cases.npz (`traj1_q`: trajectory.json's 16 control
points, 15 s); the Nextage limits are the URDF's (ikgrasp/data/nextage_actuation.json).

  ref15       the recorded trajectory, T = 15 s, S = 33, URDF limits
  fast        the same points at T = 0.6 s: speed-bound
  torque_pos  the same points at T = 1 s, velocity unlimited, every effort x 0.2: the torque binds
              (torque_scale > 1) at an entry with d > 0
  torque_neg  the same, with joint NEG_JOINT's effort lowered instead until it binds at an entry with d < 0
  static      T = 15 s, the effort of the right shoulder (RARM_JOINT1, joint 10) below its gravity torque: n_static > 0
  two         S = 2: the two ends of a seeded curve (the recorded trajectory rests at both ends, where
              every speed ties at 0 up to rounding)
  spw5        S = 33 run with samples_per_wave 5: ragged lane groups and a ragged last run
  trio        three curves whose neighbours differ (the trajectory, its points reversed, a seeded curve)
  family      mixed_17 of tests/dynamics_family_cases.py (nq = 17: 32 lanes per sample) with
              seeded_inertias, a seeded degree-6 curve inside its joint limits
  five        a seeded 5-point curve: the lower bound of n_points

Per case `<name>.`: points [B,n,nq], range (t_min, t_max, mult), S, spw, vlim, elim [nq] (1e30 =
unlimited), model; the float64 oracle's tau, g [B,S,nq], ratios [B], args [B,2], n_static [B]; `<out>_mp`
the 50-digit answers rounded to float64; dev_<out> the float64 oracle's largest deviation from them
relative to max_<out> = max|out_mp| (for a ratio over the per-entry array [B,S,nq], see
trajdyn_oracle.py); the kernel's bar is 20 x dev x max.
torque_pos / torque_neg also hold the scaling law's figures: scale = max(speed_scale, torque_scale) of
the float64 oracle, t_max_scaled = t_min + scale T, and scale_dev = the deviation from 1 of
max(speed_scale, torque_scale) evaluated at t_max_scaled in 50 digits (bar: 20 x).

Asserted here (conditions on the float64 oracle alone, met by the choice of the parameters below):
every arg's runner-up lies at least 1e-6 relative below the winner (a winner of exactly 0 ties in
every arithmetic and is pinned by the tie rule); both signs of the binding d occur across
torque_pos and torque_neg and the binding denominator E - sign(d) g is >= 0.1 E; static has
n_static > 0 and its static entries are left out of torque_scale; fast is speed-bound.
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

import dynamics_oracle as do  # noqa: E402
import trajdyn_oracle as to  # noqa: E402
from ikgrasp.model import load_nextage_actuation  # noqa: E402

OUT = to.FIXTURE
NO = to.NO_LIMIT
NEG_JOINT, NEG_EFFORT = 10, 14.0  # torque_neg: the joint whose effort is lowered (RARM_JOINT1), and to what
SHOULDER, SHOULDER_EFFORT = 10, 8.0  # static: below |g| = 10.26 N m of the recorded trajectory's sample 6


def seeded_curve(model, n_points, seed, spread=0.6):
    """control points inside the middle `spread` of the joint ranges (the curve stays in their hull)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(model.lower, -2.0), np.minimum(model.upper, 2.0)
    mid, half = 0.5 * (lo + hi), 0.5 * spread * (hi - lo)
    return mid + half * rng.uniform(-1.0, 1.0, (n_points, model.nq))


def plan():
    """-> list of (name, model name, points [B,n,nq], t_max, S, spw, vlim, elim)"""
    nx, _ = to.model_of("nextage")
    fam, _ = to.model_of("mixed_17")
    act = load_nextage_actuation()
    P = np.load(os.path.join(HERE, "rollout_cases.npz"))["traj1_q"]
    V, E = act.velocity, act.effort
    free = np.full(nx.nq, NO)
    e_neg = E.copy()
    e_neg[NEG_JOINT] = NEG_EFFORT
    e_static = E.copy()
    e_static[SHOULDER] = SHOULDER_EFFORT
    trio = np.stack([P, P[::-1], seeded_curve(nx, len(P), 11)])
    return [
        ("ref15", "nextage", P[None], 15.0, 33, 0, V, E),
        ("fast", "nextage", P[None], 0.6, 33, 0, V, E),
        ("torque_pos", "nextage", P[None], 1.0, 33, 0, free, 0.2 * E),
        ("torque_neg", "nextage", P[None], 1.0, 33, 0, free, e_neg),
        ("static", "nextage", P[None], 15.0, 33, 0, V, e_static),
        ("two", "nextage", seeded_curve(nx, len(P), 14)[None], 4.0, 2, 0, V, E),
        ("spw5", "nextage", P[None], 5.0, 33, 5, V, E),
        ("trio", "nextage", trio, 3.0, 17, 0, V, E),
        ("family", "mixed_17", seeded_curve(fam, 7, 12)[None], 2.0, 9, 0, np.full(fam.nq, 1.5), np.full(fam.nq, 40.0)),
        ("five", "nextage", seeded_curve(nx, 5, 13)[None], 2.0, 9, 0, V, E),
    ]


_trees = {}


def _tree(ar, model):
    if (ar, model) not in _trees:
        m, bi = to.model_of(model)
        _trees[(ar, model)] = do.Tree(ar, m, bi)
    return _trees[(ar, model)]


def _curve(args):
    """one curve in both arithmetics -> (float64 entries, 50-digit entries rounded to float64)"""
    model, points, t_max, S, vlim, elim = args
    e64 = to.entries(do.F64, _tree(do.F64, model), points, 0.0, t_max, 1.0, S, vlim, elim)
    emp = to.entries(do.MP, _tree(do.MP, model), points, 0.0, t_max, 1.0, S, vlim, elim)
    emp = {k: (v if k == "static" else do.to_f64(v)) for k, v in emp.items()}
    return e64, emp


def build():
    cases = plan()
    jobs = [(model, pts[b], t_max, S, vlim, elim) for (_, model, pts, t_max, S, _, vlim, elim) in cases
            for b in range(len(pts))]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(_curve, jobs)
        out = {"names": np.array([c[0] for c in cases])}
        at = 0
        binding = {}
        for name, model, pts, t_max, S, spw, vlim, elim in cases:
            B = len(pts)
            e64 = [r[0] for r in res[at:at + B]]
            emp = [r[1] for r in res[at:at + B]]
            at += B
            d = {"points": pts, "range": np.array([0.0, t_max, 1.0]), "S": np.int32(S), "spw": np.int32(spw),
                 "vlim": np.asarray(vlim, dtype=np.float64), "elim": np.asarray(elim, dtype=np.float64),
                 "model": np.array(model)}
            f64, fmp = [to.fold(e) for e in e64], [to.fold(e) for e in emp]
            for key in to.SAMPLE:
                d[key] = np.stack([e[key] for e in e64])
                d[key + "_mp"] = np.stack([e[key] for e in emp])
            for key in to.RATIOS:
                d[key] = np.array([f[key] for f in f64])
                d[key + "_mp"] = np.array([f[key] for f in fmp])
                d[to.ARGS[key]] = np.array([f[to.ARGS[key]] for f in f64], dtype=np.int32).reshape(B, 2)
            d["n_static"] = np.array([f["n_static"] for f in f64], dtype=np.int32)
            for key in to.SAMPLE + to.RATIOS:
                a64, amp = np.stack([e[key] for e in e64]), np.stack([e[key] for e in emp])
                top = float(np.abs(amp).max())
                d["max_" + key] = np.float64(top)
                d["dev_" + key] = np.float64(np.abs(a64 - amp).max() / top) if top > 0 else np.float64(0.0)
            # ---- conditions on the float64 oracle
            for b in range(B):
                assert [fmp[b][to.ARGS[k]] for k in to.RATIOS] == [f64[b][to.ARGS[k]] for k in to.RATIOS], name
                assert fmp[b]["n_static"] == f64[b]["n_static"], name
                for key in to.RATIOS:
                    gap = to.arg_gap(e64[b], key)
                    assert gap >= to.ARG_GAP, (name, b, key, gap)
            sk, sj = f64[0]["arg_torque_scale"]
            dd, gg = float(e64[0]["d"][sk, sj]), float(e64[0]["g"][sk, sj])
            binding[name] = (dd, (elim[sj] - gg if dd > 0 else elim[sj] + gg) / elim[sj], f64[0])
            print(f"{name:10s} B={B} S={S}", {k: f"{d[k][0]:.4g}@{tuple(d[to.ARGS[k]][0])}" for k in to.RATIOS},
                  "n_static", d["n_static"].tolist(),
                  "dev", {k: f"{float(d['dev_' + k]):.1e}" for k in to.SAMPLE + to.RATIOS})
            out.update({f"{name}.{k}": np.asarray(v) for k, v in d.items()})
        f = binding["fast"][2]
        assert f["speed_scale"] > 1.0 and f["speed_scale"] > f["torque_scale"], "fast is not speed-bound"
        for name in ("torque_pos", "torque_neg"):
            dd, den, f = binding[name]
            assert f["speed_scale"] == 0.0 and f["torque_scale"] > 1.0, (name, "the torque does not bind")
            assert den >= 0.1, (name, "binding denominator", den)
        assert binding["torque_pos"][0] > 0 > binding["torque_neg"][0], "the binding d needs both signs"
        f = binding["static"][2]
        sk, sj = f["arg_torque_scale"]
        assert f["n_static"] > 0 and f["static_use"] >= 1.0 and abs(float(out["static.g"][0, sk, sj])) < SHOULDER_EFFORT
        # ---- the scaling law: torque_pos / torque_neg again at t_max' = t_min + scale T, in 50 digits
        law = []
        for name in ("torque_pos", "torque_neg"):
            scale = max(float(out[name + ".speed_scale"][0]), float(out[name + ".torque_scale"][0]))
            t_scaled = 0.0 + scale * float(out[name + ".range"][1])
            out[name + ".scale"], out[name + ".t_max_scaled"] = np.float64(scale), np.float64(t_scaled)
            c = next(c for c in cases if c[0] == name)
            law.append((c[1], c[2][0], t_scaled, c[4], c[6], c[7]))
        for name, (e64, emp) in zip(("torque_pos", "torque_neg"), pool.map(_curve, law)):
            fmp = to.fold(emp)
            out[name + ".scale_dev"] = np.float64(abs(max(fmp["speed_scale"], fmp["torque_scale"]) - 1.0))
            print(f"{name}: scale {float(out[name + '.scale']):.6g}, at t_max' the 50-digit scale deviates from 1 by "
                  f"{float(out[name + '.scale_dev']):.2e} (float64 oracle: "
                  f"{abs(max(to.fold(e64)['speed_scale'], to.fold(e64)['torque_scale']) - 1.0):.2e})")
    return out


def main():
    out = build()
    if "--check" in sys.argv[1:]:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for key in out:
            assert old[key].dtype == out[key].dtype and old[key].tobytes() == out[key].tobytes(), key
        print("trajdyn_cases.npz reproduces bit for bit:", len(out), "arrays")
        return
    np.savez_compressed(OUT, **out)
    print("wrote trajdyn_cases.npz:", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
