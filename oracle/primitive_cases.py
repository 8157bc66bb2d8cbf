"""Shape pairs whose separation is known by construction -- test infrastructure
only (tests/golden/make_golden.py `primitives`, tests/test_primitives.py,
tests/test_gpu_primitives.py).  Nothing here touches the product.

Construction.  On shape A, placed at (R_A, t_A), take a surface point p_a and a
unit vector n of A's normal cone at p_a (sphere: any direction; box: a face
normal, a positive combination of the two face normals at an edge or of the
three at a vertex; cylinder: radial on the side, +-e_z on a cap, a positive
combination of both on a rim).  Take (p_b, n_b) on B the same way, a rotation
R_B with R_B n_b = -R_A n (composed with a spin about that axis) and

    t_B(g) = (R_A p_a + t_A) + g R_A n - R_B p_b.

For g > 0 the distance is exactly g: A lies below the plane through R_A p_a +
t_A with normal R_A n, B above the parallel plane at height g (lower bound),
and the two points are g apart (upper bound).  For g < 0 the midpoint of the
two points lies inside both shapes as long as |g| is small against the
dimensions (|g| <= 1e-3 m, dimensions >= 0.015 m; every normal weight >= 0.2).

A row stores the base pose (kinds, dims, R_A, t_A, R_B, c = R_A p_a + t_A,
n = R_A n, rb = R_B p_b); `placement_b` expands a gap.  Concentric rows
(n = 0, rb = 0, c = t_A: t_B = t_A for every g) are penetration-only.
"""
from __future__ import annotations

import math

import numpy as np

from . import collision_oracle as co
from . import ik_oracle as ik

SPHERE, BOX, CYLINDER, MESHBOX = co.SPHERE, co.BOX, co.CYLINDER, co.MESHBOX
KINDS = (SPHERE, BOX, CYLINDER, MESHBOX)
KIND_NAMES = {SPHERE: "sphere", BOX: "box", CYLINDER: "cylinder", MESHBOX: "meshbox"}
# feature codes
ANY, FACE, EDGE, VERTEX, SIDE, CAP, RIM, CENTRE = range(8)
FEATURES = {SPHERE: (ANY,), BOX: (FACE, EDGE, VERTEX), MESHBOX: (FACE, EDGE, VERTEX), CYLINDER: (SIDE, CAP, RIM)}
# pose tags
RANDOM, SPIN0, COAXIAL, DIAGONAL, CONCENTRIC = range(5)

GAPS_SEP = np.array([1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9])
GAPS_PEN = -np.array([1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9])
SLAB = np.array([0.15, 0.015, 0.06])  # a slab-thin box like the scene's obstacle
N_POSES = 12  # per feature pair; pose 10 is the spin-0 pose, pose 11 the slab (boxes)


def rand_rot(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def rand_dims(kind, rng):
    lu = lambda lo, hi: float(np.exp(rng.uniform(math.log(lo), math.log(hi))))
    if kind == SPHERE:
        return np.array([rng.uniform(0.03, 0.08), 0.0, 0.0])
    if kind == CYLINDER:
        return np.array([rng.uniform(0.03, 0.08), lu(0.015, 0.3), 0.0])
    return np.array([lu(0.015, 0.3), lu(0.015, 0.3), lu(0.015, 0.3)])


def _unit(v):
    return v / np.linalg.norm(v)


def _perp(n):
    t = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    return _unit(np.cross(n, t))


def feature(kind, dims, feat, rng, tag=RANDOM):
    """(p, n, u) in the shape's frame: a surface point, a unit vector of its
    normal cone, a canonical unit tangent (the edge / axis direction where the
    feature has one)."""
    sgn = lambda k=None: rng.choice([-1.0, 1.0], size=k)
    if kind == SPHERE:
        n = _unit(rng.normal(size=3))
        return dims[0] * n, n, _perp(n)
    if kind == CYLINDER:
        r, h = dims[0], dims[1]
        phi = rng.uniform(0, 2 * math.pi)
        rad = np.array([math.cos(phi), math.sin(phi), 0.0])
        ez = np.array([0.0, 0.0, 1.0])
        if feat == SIDE:
            return r * rad + rng.uniform(-0.8, 0.8) * h * ez, rad, ez
        s = sgn()
        if feat == CAP:
            rho = 0.0 if tag == COAXIAL else 0.8 * r * math.sqrt(rng.uniform())
            return rho * rad + s * h * ez, s * ez, np.array([1.0, 0.0, 0.0])
        assert feat == RIM
        a, b = rng.uniform(0.2, 1.0, 2)
        return r * rad + s * h * ez, _unit(a * rad + b * s * ez), np.array([-rad[1], rad[0], 0.0])
    h = np.asarray(dims, dtype=np.float64)
    E = np.eye(3)
    if feat == FACE:
        i = int(rng.integers(3))
        s = sgn()
        p = rng.uniform(-0.8, 0.8, 3) * h
        p[i] = s * h[i]
        return p, s * E[i], E[(i + 1) % 3]
    if feat == EDGE:
        k = int(rng.integers(3))
        i, j = (k + 1) % 3, (k + 2) % 3
        si, sj = sgn(2)
        p = np.zeros(3)
        p[k] = rng.uniform(-0.8, 0.8) * h[k]
        p[i], p[j] = si * h[i], sj * h[j]
        a, b = rng.uniform(0.2, 1.0, 2)
        return p, _unit(a * si * E[i] + b * sj * E[j]), E[k]
    assert feat == VERTEX
    s = sgn(3)
    p = s * h
    n = _unit(p) if tag == DIAGONAL else _unit(rng.uniform(0.2, 1.0, 3) * s)
    return p, n, _perp(n)


def place_b(RA, tA, fa, fb, spin):
    """R_B, c, n, rb of the construction from the two features (p, n, u)."""
    pa, na, ua = fa
    pb, nb, ub = fb
    nw, uw = RA @ na, RA @ ua
    vw = np.cross(nw, uw)
    u2 = math.cos(spin) * uw + math.sin(spin) * vw
    T = np.stack([u2, np.cross(-nw, u2), -nw], axis=1)
    Fb = np.stack([ub, np.cross(nb, ub), nb], axis=1)
    RB = T @ Fb.T
    return RB, RA @ pa + tA, nw, RB @ pb


def placement_b(row_c, row_n, row_rb, g):
    """t_B of the rows at gap g (arrays [N,3]; g scalar or [N])."""
    return row_c + np.asarray(g).reshape(-1, 1) * row_n - row_rb


# ---------------------------------------------------------------- fixture
def palettes(rng):
    """A palette: N_POSES world-fixed shapes per kind on a 2 m grid (entry 10
    axis-aligned, entry 11 of the boxes the slab); B palette: the target
    shapes, one scene each."""
    grid = [np.array([x, y, z], dtype=np.float64) for z in (-2, 0, 2) for y in (-3, -1, 1, 3) for x in (-3, -1, 1, 3)]
    pal = []
    for kind in KINDS:
        for j in range(N_POSES):
            dims = SLAB.copy() if (j == 11 and kind in (BOX, MESHBOX)) else rand_dims(kind, rng)
            R = np.eye(3) if j == 10 else rand_rot(rng)
            pal.append((kind, dims, R, grid[len(pal)]))
    bpal = [(SPHERE, rand_dims(SPHERE, rng)), (BOX, rand_dims(BOX, rng)), (BOX, SLAB.copy()),
            (CYLINDER, rand_dims(CYLINDER, rng)), (CYLINDER, np.array([0.03, 0.25, 0.0])),
            (MESHBOX, np.array([0.05, 0.05, 0.05]))]
    return pal, bpal


def _row(ka, da, RA, tA, kb, db, fa_code, fb_code, tag, rng, ia, ib):
    if tag == CONCENTRIC:
        RB, c, n, rb = rand_rot(rng), tA.copy(), np.zeros(3), np.zeros(3)
    else:
        fa = feature(ka, da, fa_code, rng, tag)
        fb = feature(kb, db, fb_code, rng, tag)
        spin = 0.0 if tag == SPIN0 else rng.uniform(0, 2 * math.pi)
        RB, c, n, rb = place_b(RA, tA, fa, fb, spin)
    return dict(kindA=ka, kindB=kb, dimsA=da, dimsB=db, RA=RA, tA=tA, RB=RB, c=c, n=n, rb=rb, featA=fa_code,
                featB=fb_code, tag=tag, ia=ia, ib=ib)


def world_rows(rng, pal, bpal):
    b_of = {k: [i for i, (kk, _) in enumerate(bpal) if kk == k] for k in KINDS}
    rows = []

    def add(ka, j, kb, jb, fa, fb, tag):
        ia = KINDS.index(ka) * N_POSES + j
        ib = b_of[kb][jb % len(b_of[kb])]
        _, da, RA, tA = pal[ia]
        rows.append(_row(ka, da, RA, tA, kb, bpal[ib][1], fa, fb, tag, rng, ia, ib))

    for ka in KINDS:
        for kb in KINDS:
            for fa in FEATURES[ka]:
                for fb in FEATURES[kb]:
                    for j in range(N_POSES):
                        add(ka, j, kb, j, fa, fb, SPIN0 if j == 10 else RANDOM)
            for j in (0, 5):  # concentric centres: the d == 0 start of both GJKs
                add(ka, j, kb, j, CENTRE, CENTRE, CONCENTRIC)
    for j in range(4):  # coaxial cap on cap
        add(CYLINDER, j, CYLINDER, j, CAP, CAP, COAXIAL)
    for ka in (BOX, MESHBOX):  # vertex on vertex along both diagonals: tight bounding spheres
        for kb in (BOX, MESHBOX):
            for j in (1, 4, 10, 11):
                add(ka, j, kb, j, VERTEX, VERTEX, DIAGONAL)
    return rows


ROBOT_JOINTS = (2, 4, 6, 8, 10, 12, 14, 0)  # head, left arm, right arm, chest
ROBOT_B = (CYLINDER, np.array([0.03, 0.03, 0.0]))
ROBOT_GAP_MAX = 1e-2  # the robot rows' sweep stops here: the arm's geometries are close to each other


def robot_rows(rng, n_q=4, per_geom=6):
    """A geometries attached to Nextage joints (two per kind), the target B a
    cylinder; world placements of A from the collision oracle's FK at seeded q.
    Every row keeps B's bounding sphere 0.02 m clear of every other A's up to
    ROBOT_GAP_MAX, so the
    scene's OR over pairs is the answer of the row's pair."""
    geoms = []
    for i, joint in enumerate(ROBOT_JOINTS):
        kind = KINDS[i % 4]
        d = rand_dims(kind, rng)
        d = np.where(d > 0, np.clip(d, 0.015, 0.04), 0.0)
        geoms.append(dict(kind=kind, joint=joint, R=rand_rot(rng), t=rng.uniform(-0.05, 0.05, 3), dims=d,
                          target=False))
    brad = lambda k, d: d[0] if k == SPHERE else math.hypot(d[0], d[1]) if k == CYLINDER else np.linalg.norm(d)
    qs = rng.uniform(np.maximum(ik.LOWER, -1.2), np.minimum(ik.UPPER, 1.2), size=(n_q, ik.NQ))
    rows = []
    for iq, q in enumerate(qs):
        poses = co.geom_poses({"geoms": geoms}, q, np.eye(3), np.zeros(3))
        for ia, g in enumerate(geoms):
            RA, tA = poses[ia]
            n_ok = 0
            for _ in range(2000):
                if n_ok == per_geom:
                    break
                fa = int(rng.choice(FEATURES[g["kind"]]))
                fb = int(rng.choice(FEATURES[ROBOT_B[0]]))
                r = _row(g["kind"], g["dims"], RA, tA, ROBOT_B[0], ROBOT_B[1], fa, fb, RANDOM, rng, ia, 0)
                tB = r["c"] - r["rb"]
                clear = min(np.linalg.norm(tB - poses[j][1]) - brad(ROBOT_B[0], ROBOT_B[1]) -
                            brad(geoms[j]["kind"], geoms[j]["dims"]) for j in range(len(geoms)) if j != ia)
                if clear < ROBOT_GAP_MAX + 0.02:
                    continue
                r["iq"] = iq
                rows.append(r)
                n_ok += 1
            assert n_ok == per_geom, (iq, ia)
    return qs, geoms, rows


def make(seed=20240611):
    rng = np.random.default_rng(seed)
    pal, bpal = palettes(rng)
    rows = world_rows(rng, pal, bpal)
    qs, rgeoms, rrows = robot_rows(rng)
    out = {}
    for prefix, rr in (("", rows), ("rob_", rrows)):
        for key in rr[0]:
            out[prefix + key] = np.array([r[key] for r in rr])
    out.update(pal_kind=np.array([p[0] for p in pal]), pal_dims=np.array([p[1] for p in pal]),
               pal_R=np.array([p[2] for p in pal]), pal_t=np.array([p[3] for p in pal]),
               bpal_kind=np.array([b[0] for b in bpal]), bpal_dims=np.array([b[1] for b in bpal]),
               rob_q=qs, rob_geom_kind=np.array([g["kind"] for g in rgeoms]),
               rob_geom_joint=np.array([g["joint"] for g in rgeoms]),
               rob_geom_R=np.array([g["R"] for g in rgeoms]), rob_geom_t=np.array([g["t"] for g in rgeoms]),
               rob_geom_dims=np.array([g["dims"] for g in rgeoms]), rob_b_kind=np.array(ROBOT_B[0]),
               rob_b_dims=ROBOT_B[1], gaps_sep=GAPS_SEP, gaps_pen=GAPS_PEN)
    return out


# ---------------------------------------------------------------- exact membership / closed forms
def local_point(R, t, x):
    return R.T @ (x - t)


def surface_residual(kind, dims, R, t, x):
    """0 when x lies on the shape's surface: max over the shape's constraints
    (positive outside, negative inside)."""
    return -depth(kind, dims, R, t, x)


def depth(kind, dims, R, t, x):
    """Radius of the largest ball about x inside the shape (negative outside,
    then minus a lower bound of the distance)."""
    l = local_point(R, t, x)
    if kind == SPHERE:
        return dims[0] - np.linalg.norm(l)
    if kind == CYLINDER:
        return min(dims[0] - math.hypot(l[0], l[1]), dims[1] - abs(l[2]))
    return float(np.min(np.asarray(dims) - np.abs(l)))


def point_cylinder_distance(dims, R, t, x):
    """Point to solid cylinder: hypot(max(rho - r, 0), max(|z| - h, 0))."""
    l = local_point(R, t, x)
    return math.hypot(max(math.hypot(l[0], l[1]) - dims[0], 0.0), max(abs(l[2]) - dims[1], 0.0))


def box_box_sat(Ra, ta, ha, Rb, tb, hb):
    """15-axis separating-axis test -> (intersecting, largest separation over
    the axes: > 0 separated by at least that much)."""
    axes = [Ra[:, i] for i in range(3)] + [Rb[:, i] for i in range(3)]
    axes += [np.cross(Ra[:, i], Rb[:, j]) for i in range(3) for j in range(3)]
    d = tb - ta
    best = -np.inf
    for ax in axes:
        nrm = np.linalg.norm(ax)
        if nrm < 1e-9:
            continue
        ax = ax / nrm
        ra = float(np.sum(ha * np.abs(Ra.T @ ax)))
        rb = float(np.sum(hb * np.abs(Rb.T @ ax)))
        best = max(best, abs(float(d @ ax)) - ra - rb)
    return best <= 0.0, best
