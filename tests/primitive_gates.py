"""Gap sweep and gates of the primitive-pair tests (tests/test_primitives.py on
the host emulator, tests/test_gpu_primitives.py through the public API)."""
import numpy as np

import helpers

from oracle import primitive_cases as pc

# gates: boolean margin, smallest gated separated gap,
# separated tolerance, intersecting tolerance = smallest gated depth
GATES = {"f64": dict(margin=1e-9, sep_min=1e-6, sep_tol=1e-7, pen_tol=1e-9),
         "f32": dict(margin=1e-4, sep_min=1e-3, sep_tol=1e-4, pen_tol=1e-4)}
# fp64 boolean of a pair with a cylinder: clearances are gated from 1e-7 m,
# the smallest decade the boolean GJK meets on every constructed row.  Below it
# the iteration ends at its cap, or on a simplex that holds the origin as far
# as its products resolve, and answers "touching" (at 1e-8 m: 16 of the 432
# box-like against cylinder rows; at 1e-9 m: 36 rows).  Penetrating
# rows of these pairs stay gated from 1e-9 m, as every other kind pair is in
# both directions.
CYLINDER_SEP_MARGIN = 1e-7


def boolean_margin(kA, kB, gap, dtype):
    """Per swept row: the clearance / depth from which the boolean is gated."""
    m = np.full(len(gap), GATES[dtype]["margin"])
    if dtype == "f64":
        m[((kA == pc.CYLINDER) | (kB == pc.CYLINDER)) & (gap > 0)] = CYLINDER_SEP_MARGIN
    return m


def sweep(fx, prefix=""):
    """Rows x gaps, flattened: (row index, g) with every separated gap for the
    constructed rows and every penetrating gap for all rows (concentric rows:
    penetration only, t_B = t_A whatever g)."""
    n = len(fx[prefix + "kindA"])
    conc = fx[prefix + "tag"] == pc.CONCENTRIC
    idx, gap = [], []
    for g in fx["gaps_sep"]:
        if prefix and g > pc.ROBOT_GAP_MAX:
            continue
        r = np.nonzero(~conc)[0]
        idx.append(r)
        gap.append(np.full(len(r), g))
    for g in fx["gaps_pen"]:
        idx.append(np.arange(n))
        gap.append(np.full(n, g))
    return np.concatenate(idx), np.concatenate(gap)


def placements(fx, idx, gap, prefix=""):
    """[N,12] placements of A and B of the swept rows (t_B by the one-line formula)."""
    f = lambda k: fx[prefix + k][idx]
    tB = pc.placement_b(f("c"), f("n"), f("rb"), gap)
    PA = np.concatenate([f("RA").reshape(-1, 9), f("tA")], axis=1)
    PB = np.concatenate([f("RB").reshape(-1, 9), tB], axis=1)
    return np.ascontiguousarray(PA), np.ascontiguousarray(PB)



def kind_pair_table(fx, idx, gap, hit, d, prefix=""):
    """Per kind pair and decade: rows, boolean errors, worst |d - g| (separated)
    or worst d (intersecting).  The report of DESIGN.md §2b / §2c."""
    kA, kB = fx[prefix + "kindA"][idx], fx[prefix + "kindB"][idx]
    out = {}
    for a in pc.KINDS:
        for b in pc.KINDS:
            m = (kA == a) & (kB == b)
            if not m.any():
                continue
            row = {}
            for g in np.unique(gap):
                s = m & (gap == g)
                if not s.any():
                    continue
                err = float(np.abs(d[s] - g).max()) if g > 0 else float(d[s].max())
                row[f"{g:+.0e}"] = [int(s.sum()), int((hit[s] != (g < 0)).sum()), float(f"{err:.2e}")]
            out[f"{pc.KIND_NAMES[a]}/{pc.KIND_NAMES[b]}"] = row
    return out


def check_gates(name, fx, idx, gap, hit, d, dtype, prefix=""):
    """The gates of part 4 on one swept answer set; returns the failures as text."""
    G = GATES[dtype]
    kA, kB = fx[prefix + "kindA"][idx], fx[prefix + "kindB"][idx]
    bad = []
    hv = hit if hit is not None else np.zeros(len(gap), dtype=bool)
    dv = d if d is not None else np.full(len(gap), np.nan)

    def note(what, m):
        if m.any():
            i = np.nonzero(m)[0]
            pairs = sorted({(pc.KIND_NAMES[a], pc.KIND_NAMES[b]) for a, b in zip(kA[i], kB[i])})
            bad.append(f"{what}: {len(i)} rows, gaps {sorted(set(gap[i]))}, kinds {pairs}, first rows "
                       f"{[(int(idx[k]), float(gap[k]), bool(hv[k]), float(dv[k])) for k in i[:5]]}")

    helpers.report(name, kind_pair_table(fx, idx, gap, hv, dv, prefix))
    if hit is not None:
        note("boolean != (g < 0)", (np.abs(gap) >= boolean_margin(kA, kB, gap, dtype)) & (hit != (gap < 0)))
    if d is not None:
        note("separated distance", (gap >= G["sep_min"]) & ~(np.abs(d - gap) <= G["sep_tol"]))
        note("intersecting distance", (gap <= -G["pen_tol"]) & ~(d <= G["pen_tol"]))
    if hit is not None and d is not None:
        both = (gap >= G["sep_min"]) | (gap <= -max(G["pen_tol"], G["margin"]))
        note("collision != (distance <= tol)", both & (hit != (d <= G["pen_tol"])))
    return bad


# ---------------------------------------------------------------- synthetic scenes
def _scene(kinds, joints, Rs, ts, dims, b_kind, b_dims):
    from ikgrasp.collision import CollisionScene, Geom
    geoms = [Geom(f"a_{i}", int(kinds[i]), int(joints[i]), f"a_{i}", np.array(Rs[i]), np.array(ts[i]),
                  np.array(dims[i])) for i in range(len(kinds))]
    geoms.append(Geom("b_0", int(b_kind), -1, "b", np.eye(3), np.zeros(3), np.array(b_dims), True))
    n = len(kinds)
    return CollisionScene(geoms, np.array([(i, n) for i in range(n)], dtype=np.int32))


def world_scene(fx, b):
    """The palette of world-fixed A shapes, each paired with target shape b of
    the B palette: pair k = (A_k, target)."""
    n = len(fx["pal_kind"])
    return _scene(fx["pal_kind"], -np.ones(n), fx["pal_R"], fx["pal_t"], fx["pal_dims"], fx["bpal_kind"][b],
                  fx["bpal_dims"][b])


def robot_scene(fx):
    """The A shapes attached to Nextage joints, each paired with the target cylinder."""
    return _scene(fx["rob_geom_kind"], fx["rob_geom_joint"], fx["rob_geom_R"], fx["rob_geom_t"],
                  fx["rob_geom_dims"], fx["rob_b_kind"], fx["rob_b_dims"])
