"""A family of synthetic dual-arm robots, one per switch of the model
compiler (csrc/ikg_model_build.hpp build_kmodel / choose_spec) and of the
hipRTC generator (csrc/ikg_jit.hip): test data written for this repository's
tests, in the way tests/golden/tilted_dualarm.urdf was written by hand.

Every member is a row of MEMBERS: link offsets at Nextage scale (0.05-0.35 m),
joint axes, limits, the two hand frames (*_EFF), passive chains, a grasp
posture q* and the tables the model compiler must give it (`expect`).
`robot_urdf` / `cube_urdf` turn a row into URDF text; the committed copies are
tests/golden/family/<member>.urdf and <member>_cube.urdf (written by
tests/golden/make_family_golden.py, compared with this generator's text in
tests/test_robot_family.py).

    member         the one switch it flips
    nx_scaled      Nextage axis pattern, identity joint rotations, the Nextage zero
                   offset components, spherical wrist -- but every length, the hand
                   yaw (0.7) and the limits differ, asymmetric between the arms;
                   nq = 13 (no passive joint)              -> kSpecNextage
    nx_extra_zero  as nx_scaled with arm joint 2's y = 0 too, different hand yaws
                   (0.7 / 0.55), three passive joints      -> kSpecNextage, zmask larger
    nx_zbreak      arm joint 2's x = 0.02                  -> kSpecGenericWrist
    nx_rot         rpy on arm joint 2 and on the root      -> kSpecGenericWrist, rot_mask
    offset_wrist   arm joint 5 offset (0, 0.03, z)         -> kSpecGeneric (6x6 QR)
    wrist_edge     arm joint 5 offset (0, 1e-13, z)        -> kSpecGeneric; 1e-17: wrist
    hand_general   general, different hand rotations       -> hand_axis 3
    hand_cross     hands rotated about X (last joint: Z)   -> hand_axis 0, no hand fold
    mixed_axes     root about Y on a rotated base, arm axes X,Z,Y,Y,Z,X (two negative,
                   one unaligned), nq = 32 with 19 passive joints before, between and
                   after the arms, right arm first in q order, no spherical wrist
"""
import copy
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILY_DIR = os.path.join(GOLDEN, "family")

# csrc/ikg_device.hpp
PATTERN_NEXTAGE = 2 | (2 << 2) | (1 << 4) | (1 << 6) | (0 << 8) | (1 << 10) | (2 << 12) | (2 << 14)
ZERO_NEXTAGE = (3 << 3) | (1 << 6) | (2 << 9) | (6 << 12) | (3 << 15)
SPEC_GENERIC, SPEC_NEXTAGE, SPEC_GENERIC_WRIST = 0, 1, 2
INFO = ("spec", "wrist", "hand_axis", "rot_mask", "zmask", "pattern", "n_passive", "nq")

X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
O = (0.0, 0.0, 0.0)


def J(xyz, axis, lo, hi, rpy=O):
    return dict(xyz=tuple(xyz), rpy=tuple(rpy), axis=tuple(axis), lo=lo, hi=hi)


def _nx():
    """The Nextage-class base row (nx_scaled)."""
    return dict(
        base=None,
        root=dict(name="CHEST_JOINT0", **J((0, 0, 1.0), Z, -1.6, 1.9)),
        arm_names=("LARM_JOINT", "RARM_JOINT"),
        arms=(
            [J((0.05, 0.15, 0.12), Z, -1.4, 1.7), J((0, 0, 0.08), Y, -2.2, 0.9), J((0, 0.11, -0.28), Y, -2.6, 0.2),
             J((0.21, 0, -0.05), X, -2.5, 2.9), J((0.17, 0, 0), Y, -1.6, 0.55), J((0, 0, -0.15), Z, -2.7, 2.8)],
            [J((0.06, -0.13, 0.10), Z, -1.7, 1.4), J((0, 0, 0.07), Y, -2.3, 1.0), J((0, -0.08, -0.22), Y, -2.7, 0.1),
             J((0.16, 0, -0.06), X, -0.4, 2.5), J((0.13, 0, 0), Y, -1.7, 1.6), J((0, 0, -0.11), Z, -2.8, 2.7)]),
        hands=(dict(xyz=(0.09, 0.06, -0.03), rpy=(0, 0, 0.7)), dict(xyz=(0.07, -0.055, -0.035), rpy=(0, 0, 0.7))),
        passive=[],  # chains hanging off the chest link: (joint name prefix, [joints])
        collisions={},
        q_star=dict(root=0.1, arms=([0.2, -0.3, -1.4, 0.1, 0.3, 0.2], [-0.2, -0.35, -1.3, -0.1, -0.3, -0.2])),
    )


def _set_arm(m, j, **kw):
    """Override fields of arm joint j on both arms: value or (left, right)."""
    for k, v in kw.items():
        for a in range(2):
            m["arms"][a][j][k] = v[a] if isinstance(v, list) else v


HEAD = ("HEAD_JOINT", [J((0, 0, 0.35), Z, -1.0, 1.2), J((0, 0.02, 0.05), Y, -0.4, 0.5)])


def _members():
    out = {}

    m = _nx()
    m["expect"] = dict(spec=SPEC_NEXTAGE, wrist=1, hand_axis=2, rot_mask=0, zmask=ZERO_NEXTAGE,
                       pattern=PATTERN_NEXTAGE, n_passive=0, nq=13)
    out["nx_scaled"] = m

    m = _nx()
    _set_arm(m, 2, xyz=[(0, 0, -0.28), (0, 0, -0.22)])
    _set_arm(m, 0, xyz=[(0.05, 0.2, 0.12), (0.06, -0.19, 0.10)])  # the shoulders take the width joint 2 lost
    m["hands"][1]["rpy"] = (0, 0, 0.55)
    m["passive"] = [HEAD, ("TORSO_CAM", [J((0.1, 0, 0.2), X, -0.3, 0.3)])]
    m["expect"] = dict(spec=SPEC_NEXTAGE, wrist=1, hand_axis=2, rot_mask=0, zmask=ZERO_NEXTAGE | (1 << 7),
                       pattern=PATTERN_NEXTAGE, n_passive=3, nq=16)
    out["nx_extra_zero"] = m

    m = _nx()
    _set_arm(m, 2, xyz=[(0.02, 0.11, -0.28), (0.02, -0.08, -0.22)])
    m["passive"] = [HEAD]
    m["expect"] = dict(spec=SPEC_GENERIC_WRIST, wrist=1, hand_axis=2, rot_mask=0, zmask=ZERO_NEXTAGE & ~(1 << 6),
                       pattern=PATTERN_NEXTAGE, n_passive=2, nq=15)
    out["nx_zbreak"] = m

    m = _nx()
    _set_arm(m, 2, rpy=[(0.0, 0.15, 0.0), (0.05, -0.1, 0.0)])
    m["root"]["rpy"] = (0.05, -0.04, 0.2)
    m["passive"] = [HEAD]
    m["expect"] = dict(spec=SPEC_GENERIC_WRIST, wrist=1, hand_axis=2, rot_mask=(1 << 2) | (1 << 6),
                       zmask=ZERO_NEXTAGE, pattern=PATTERN_NEXTAGE, n_passive=2, nq=15)
    out["nx_rot"] = m

    m = _nx()
    _set_arm(m, 5, xyz=[(0, 0.03, -0.15), (0, 0.03, -0.11)])
    m["passive"] = [HEAD]
    m["collisions"] = {
        "CHEST_Link": [("box", dict(size="0.2 0.3 0.3"), (0, 0, 0.15), O)],
        "HEAD_JOINT_Link0": [("sphere", dict(radius="0.08"), (0, 0, 0.1), O)],
        "LARM_JOINT_Link2": [("cylinder", dict(radius="0.04", length="0.2"), (0, 0, -0.12), O)],
        "RARM_JOINT_Link2": [("cylinder", dict(radius="0.04", length="0.16"), (0, 0, -0.1), O)],
        "LARM_JOINT_Link5": [("box", dict(size="0.05 0.06 0.07"), (0, 0, -0.05), (0.1, 0.2, 0))],
        "RARM_JOINT_Link5": [("box", dict(size="0.05 0.06 0.07"), (0, 0, -0.05), (-0.1, 0.2, 0))],
    }
    m["expect"] = dict(spec=SPEC_GENERIC, wrist=0, hand_axis=2, rot_mask=0, zmask=ZERO_NEXTAGE & ~(1 << 16),
                       pattern=PATTERN_NEXTAGE, n_passive=2, nq=15)
    out["offset_wrist"] = m

    m = _nx()
    _set_arm(m, 5, xyz=[(0, 1e-13, -0.15), (0, 1e-13, -0.11)])
    m["passive"] = [HEAD]
    m["expect"] = dict(spec=SPEC_GENERIC, wrist=0, hand_axis=2, rot_mask=0, zmask=ZERO_NEXTAGE & ~(1 << 16),
                       pattern=PATTERN_NEXTAGE, n_passive=2, nq=15)
    out["wrist_edge"] = m

    m = _nx()
    m["hands"] = (dict(xyz=(0.09, 0.06, -0.03), rpy=(0.3, -0.2, 0.9)), dict(xyz=(0.07, -0.055, -0.035), rpy=(-0.25, 0.35, 0.5)))
    m["passive"] = [HEAD]
    m["expect"] = dict(spec=SPEC_GENERIC_WRIST, wrist=1, hand_axis=3, rot_mask=0, zmask=ZERO_NEXTAGE,
                       pattern=(PATTERN_NEXTAGE & ~(3 << 14)) | (3 << 14), n_passive=2, nq=15)
    out["hand_general"] = m

    m = _nx()
    m["hands"] = (dict(xyz=(0.09, 0.06, -0.03), rpy=(0.6, 0, 0)), dict(xyz=(0.07, -0.055, -0.035), rpy=(-0.45, 0, 0)))
    m["passive"] = [HEAD]
    m["expect"] = dict(spec=SPEC_GENERIC_WRIST, wrist=1, hand_axis=0, rot_mask=0, zmask=ZERO_NEXTAGE,
                       pattern=PATTERN_NEXTAGE & ~(3 << 14), n_passive=2, nq=15)
    out["hand_cross"] = m

    # mixed_axes: children of the chest link in joint-name order: AA_* (10 passive,
    # serial), ARM_A_* (the RIGHT arm), M_* (5 passive), N_ARM_* (the left arm),
    # T_* (4 passive): nq = 1 + 10 + 6 + 5 + 6 + 4
    def chain(n, seed):
        rng = np.random.default_rng(seed)
        axes = (X, Y, Z, (0, -1, 0), (0.6, 0, 0.8))
        return [J(tuple(np.round(rng.uniform(-0.06, 0.06, 3), 3)), axes[k % 5], -0.5 - 0.05 * k, 0.4 + 0.05 * k,
                  rpy=(0.1 * (k % 3), 0, -0.1 * (k % 2))) for k in range(n)]

    m = dict(
        base=((0.1, -0.05, 0.3), (0.02, -0.03, 0.4)),  # rpy, xyz of the base placement
        root=dict(name="BODY_JOINT", **J((0, 0, 0.6), Y, -1.2, 1.5, rpy=(0.0, 0.0, 0.1))),
        arm_names=("N_ARM_JOINT", "ARM_A_JOINT"),
        arms=(
            [J((0.05, 0.16, 0.12), X, -1.9, 1.6, rpy=(0, 0, 0.2)), J((0.02, 0.05, 0.09), (0, 0, -1), -1.8, 1.9),
             J((0.22, 0.03, -0.04), (0.0, 0.8, 0.6), -2.4, 2.2), J((0.04, 0.02, -0.21), Y, -2.6, 2.5),
             J((0.03, 0.12, 0.02), Z, -2.0, 2.1, rpy=(0.1, 0, 0)), J((0.02, 0.03, -0.1), (-1, 0, 0), -2.7, 2.8)],
            [J((0.06, -0.14, 0.10), X, -1.6, 1.9, rpy=(0, 0, -0.2)), J((0.02, -0.05, 0.08), (0, 0, -1), -1.9, 1.8),
             J((0.19, -0.03, -0.05), (0.28, 0.96, 0.0), -2.2, 2.4), J((0.05, -0.02, -0.18), Y, -2.5, 2.6),
             J((0.03, -0.1, 0.02), Z, -2.1, 2.0, rpy=(-0.1, 0, 0)), J((0.02, -0.03, -0.09), (-1, 0, 0), -2.8, 2.7)]),
        hands=(dict(xyz=(0.08, 0.05, -0.03), rpy=(0.3, -0.2, 0.9)), dict(xyz=(0.07, -0.05, -0.03), rpy=(-0.2, 0.3, -0.8))),
        passive=[("AA_JOINT", chain(10, 1)), ("M_JOINT", chain(5, 2)), ("T_JOINT", chain(4, 3))],
        collisions={},
        q_star=dict(root=0.1, arms=([0.3, 0.4, -0.9, 0.2, 0.3, 0.2], [-0.3, -0.4, -0.8, 0.3, -0.3, -0.2])),
    )
    m["expect"] = dict(spec=SPEC_GENERIC, wrist=0, hand_axis=3, rot_mask=127, zmask=0,
                       pattern=1 | (0 << 2) | (2 << 4) | (1 << 6) | (1 << 8) | (2 << 10) | (0 << 12) | (3 << 14),
                       n_passive=19, nq=32)
    out["mixed_axes"] = m
    return out


MEMBERS = _members()
NAMES = tuple(MEMBERS)
THREE_FRAME = ("nx_scaled", "offset_wrist", "mixed_axes")  # members with WORLD / LOCAL / LWA fixtures
DAMPED = ("nx_scaled", "offset_wrist")  # members with damped (lam = 1e-6) oracle fixtures
COLLISION = "offset_wrist"


def wrist_edge_variant(eps):
    """wrist_edge with arm joint 5's sideways offset = eps (model check only)."""
    m = copy.deepcopy(MEMBERS["wrist_edge"])
    _set_arm(m, 5, xyz=[(0, eps, -0.15), (0, eps, -0.11)])
    return m


# ---------------------------------------------------------------- URDF text
def _v(t):
    return " ".join(repr(float(x)) for x in t)


def _origin(xyz, rpy):
    return f'<origin xyz="{_v(xyz)}"' + (f' rpy="{_v(rpy)}"' if tuple(rpy) != O else "") + "/>"


def _revolute(name, parent, child, j):
    return [f'  <joint name="{name}" type="revolute"><parent link="{parent}"/><child link="{child}"/>',
            f'    {_origin(j["xyz"], j["rpy"])}<axis xyz="{_v(j["axis"])}"/>'
            f'<limit lower="{j["lo"]!r}" upper="{j["hi"]!r}"/></joint>']


def robot_urdf(name, m=None):
    """URDF text of a member: links (with the member's collision primitives),
    revolute and fixed joints, origins, axes, limits, LARM_EFF / RARM_EFF."""
    m = MEMBERS[name] if m is None else m
    links, joints = ["base_link", "CHEST_Link"], []
    joints += _revolute(m["root"]["name"], "base_link", "CHEST_Link", m["root"])
    for prefix, chain in m["passive"]:
        parent = "CHEST_Link"
        for k, j in enumerate(chain):
            child = f"{prefix}_Link{k}"
            links.append(child)
            joints += _revolute(f"{prefix}{k}", parent, child, j)
            parent = child
    for a, side in enumerate("LR"):
        prefix, parent = m["arm_names"][a], "CHEST_Link"
        for k, j in enumerate(m["arms"][a]):
            child = f"{prefix}_Link{k}"
            links.append(child)
            joints += _revolute(f"{prefix}{k}", parent, child, j)
            parent = child
        links.append(f"{side}ARM_EFF_Link")
        h = m["hands"][a]
        joints += [f'  <joint name="{side}ARM_EFF" type="fixed"><parent link="{parent}"/><child link="{side}ARM_EFF_Link"/>',
                   f'    {_origin(h["xyz"], h["rpy"])}</joint>']
    out = ['<?xml version="1.0"?>',
           f'<!-- Synthetic dual-arm robot "{name}" of the test family (tests/robot_family.py); written',
           '     for this repository\'s tests by tests/golden/make_family_golden.py, not a reference file. -->',
           f'<robot name="{name}">']
    for l in links:
        cols = "".join(f'<collision>{_origin(xyz, rpy)}<geometry><{tag} '
                       + " ".join(f'{k}="{v}"' for k, v in attrs.items()) + "/></geometry></collision>"
                       for tag, attrs, xyz, rpy in m["collisions"].get(l, []))
        out.append(f'  <link name="{l}">{cols}</link>' if cols else f'  <link name="{l}"/>')
    return "\n".join(out + joints + ["</robot>"]) + "\n"


def base_placement(name, m=None):
    """(R, t) premultiplied into the root joint's placement, or None."""
    from oracle import ik_oracle as ik
    m = MEMBERS[name] if m is None else m
    if m["base"] is None:
        return None
    rpy, xyz = m["base"]
    return ik.urdf_rpy_to_matrix(*rpy), np.array(xyz, dtype=np.float64)


def _rpy(R):
    """URDF rpy of a rotation (R = Rz(y) Ry(p) Rx(r))."""
    return np.arctan2(R[2, 1], R[2, 2]), np.arcsin(-R[2, 0]), np.arctan2(R[1, 0], R[0, 0])


def chain_model(name, m=None):
    """The raw-axis oracle's model of a member (oracle/generic_oracle.py), from the generator's text."""
    from oracle import generic_oracle as go
    return go.ChainModel(robot_urdf(name, m), base_placement(name, m))


def q_star(name, cm=None):
    """The grasp posture in q order (passive joints at 0)."""
    m = MEMBERS[name]
    cm = chain_model(name) if cm is None else cm
    q = np.zeros(cm.nq)
    q[cm.names.index(m["root"]["name"])] = m["q_star"]["root"]
    for a in range(2):
        for k, v in enumerate(m["q_star"]["arms"][a]):
            q[cm.names.index(f'{m["arm_names"][a]}{k}')] = v
    return q


def grasp_center(name, cm=None):
    cm = chain_model(name) if cm is None else cm
    oMi = cm.fk(q_star(name, cm))
    return 0.5 * (cm.frame(oMi, "LARM_EFF")[1] + cm.frame(oMi, "RARM_EFF")[1])


def cube_urdf(name):
    """The member's grasp object, built as tests/golden/make_golden.py's
    make_generic_cases builds tilted_cube.urdf: the hook frames are the hands
    at q* seen from an unrotated cube frame midway between them."""
    cm = chain_model(name)
    oMi = cm.fk(q_star(name, cm))
    hands = [cm.frame(oMi, h) for h in ("LARM_EFF", "RARM_EFF")]
    center = 0.5 * (hands[0][1] + hands[1][1])
    lines = ['<?xml version="1.0"?>',
             f'<!-- Grasp object of the family robot "{name}" (tests/robot_family.py): hook frames = the hands',
             '     at the posture q* seen from a cube frame between them. -->',
             f'<robot name="{name}_cube">', '  <link name="base_link"/>']
    for h, (R, t) in zip(("LARM_HOOK", "RARM_HOOK"), hands):
        lines += [f'  <link name="{h}_link"/>',
                  f'  <joint name="{h}" type="fixed"><parent link="base_link"/><child link="{h}_link"/>',
                  f'    <origin xyz="{_v(t - center)}" rpy="{_v(_rpy(R))}"/></joint>']
    return "\n".join(lines + ["</robot>"]) + "\n"


def paths(name):
    return os.path.join(FAMILY_DIR, f"{name}.urdf"), os.path.join(FAMILY_DIR, f"{name}_cube.urdf")


def load_model(name):
    """The product's compiled model (ikgrasp.model.DualArmModel) of the committed URDFs."""
    from ikgrasp.model import DualArmModel
    robot, cube = paths(name)
    return DualArmModel.from_urdf(robot, cube, base_placement(name))


def load_cases():
    """family_cases.npz as {member: {key: array}} plus the shared entries under ''."""
    d = dict(np.load(os.path.join(GOLDEN, "family_cases.npz")))
    out = {n: {} for n in NAMES}
    out[""] = {}
    for k, v in d.items():
        n = next((n for n in sorted(NAMES, key=len, reverse=True) if k.startswith(n + ".")), "")
        out[n][k[len(n) + 1:] if n else k] = v
    for n in THREE_FRAME:  # entries the generator leaves out (make_family_golden.py)
        c = out[n]
        c["fk_J"] = c["J_rf1"]
        for r in (0, 1, 2):
            c[f"placement_rf{r}"] = c["fk_hands"]
            c[f"velocity_rf{r}"] = np.einsum("bij,bj->bi", c[f"J_rf{r}"], c["fk_v"]).reshape(-1, 2, 6)
            c[f"dJv_rf{r}"] = np.einsum("bij,bj->bi", c[f"dJ_rf{r}"], c["fk_v"])
    return out


def collision_scene(model, table=(0.65, 0.0, 1.2)):
    """offset_wrist's scene, as test_gpu_jit.py's _tilted_scene: the URDF's
    collision primitives, a world-fixed table box and the 0.1 m grasp cube at
    each solve's target; every pair of geometries on different joints.  The table
    stands beside and below the grasp (centre 0.25, 0.09, 1.36), where it meets the
    hands or the cube in some of the 24 cases and not in others."""
    import xml.etree.ElementTree as ET

    from ikgrasp.collision import BOX, CollisionScene, Geom, _link_geoms, _robot_link_frames
    root = ET.parse(paths(COLLISION)[0]).getroot()
    geoms = _link_geoms(root, _robot_link_frames(root, model.joint_names, model.axis_frames()))
    geoms.append(Geom("table_0", BOX, -1, "table", np.eye(3), np.array(table, dtype=np.float64),
                      np.array([0.3, 0.6, 0.05])))
    geoms.append(Geom("cube_0", BOX, -1, "cube", np.eye(3), np.zeros(3), np.array([0.05, 0.05, 0.05]), True))
    n = len(geoms)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if geoms[i].joint != geoms[j].joint]
    return CollisionScene(geoms, np.array(pairs, dtype=np.int32))


# ---------------------------------------------------------------- three-frame kinematics on raw axes
def _act(M, m):
    R, p = M
    w = R @ m[3:]
    return np.concatenate([R @ m[:3] + np.cross(p, w), w])


def _act_inv(M, m):
    R, p = M
    return np.concatenate([R.T @ (m[:3] - np.cross(p, m[3:])), R.T @ m[3:]])


def _mcross(a, b):
    return np.concatenate([np.cross(a[3:], b[:3]) + np.cross(a[:3], b[3:]), np.cross(a[3:], b[3:])])


def frame_kinematics(cm, q, v, rf):
    """oracle/control_oracle.py's frame_kinematics (Pinocchio's spatial-algebra
    formulation: J_i = oMi.act(S_i), dJ_i = ov_i x J_i, then the frame's rf)
    on a raw-axis ChainModel: S_i = [0; e_i] for the URDF's unit axis e_i,
    joint rotations by Rodrigues.  rf: 0 WORLD, 1 LOCAL, 2 LOCAL_WORLD_ALIGNED.
    Layout of ikg_frame_kinematics_batch."""
    from oracle import generic_oracle as go
    from oracle import ik_oracle as ik
    nq = cm.nq
    oMi, vl, ov = [], [], []
    for j in range(nq):
        R0, t0 = cm.placement[j]
        li = (R0 @ go.rodrigues(cm.axis[j], q[j]), t0.copy())
        vj = np.concatenate([np.zeros(3), cm.axis[j]]) * v[j]
        p = cm.parent[j]
        if p >= 0:
            vj = vj + _act_inv(li, vl[p])
        oMi.append(li if p < 0 else ik.se3_mul(oMi[p], li))
        vl.append(vj)
        ov.append(_act(oMi[j], vj))
    out = {"placement": np.zeros((2, 12)), "velocity": np.zeros((2, 6)), "J": np.zeros((12, nq)),
           "dJ": np.zeros((12, nq)), "dJv": np.zeros(12)}
    for h, name in enumerate(("LARM_EFF", "RARM_EFF")):
        j, fM = cm.frames[name]
        oMf = ik.se3_mul(oMi[j], fM)
        Rw, p = oMf
        v_f = _act_inv(fM, vl[j])
        Jh, dJh = np.zeros((6, nq)), np.zeros((6, nq))
        i = j
        while i >= 0:
            Jw = _act(oMi[i], np.concatenate([np.zeros(3), cm.axis[i]]))
            dJw = _mcross(ov[i], Jw)
            if rf == 0:
                Jh[:, i], dJh[:, i] = Jw, dJw
            elif rf == 2:
                Jh[:, i] = np.concatenate([Jw[:3] - np.cross(p, Jw[3:]), Jw[3:]])
                d = np.concatenate([dJw[:3] - np.cross(p, dJw[3:]), dJw[3:]])
                d[:3] -= np.cross(ov[j][:3] + np.cross(ov[j][3:], p), Jw[3:])
                dJh[:, i] = d
            else:
                Jl = _act_inv(oMf, Jw)
                Jh[:, i] = Jl
                dJh[:, i] = _act_inv(oMf, dJw) - _mcross(v_f, Jl)
            i = cm.parent[i]
        vel = v_f if rf == 1 else (np.concatenate([Rw @ v_f[:3], Rw @ v_f[3:]]) if rf == 2 else _act(oMf, v_f))
        out["placement"][h] = np.concatenate([Rw.reshape(9), p])
        out["velocity"][h] = vel
        out["J"][6 * h:6 * h + 6] = Jh
        out["dJ"][6 * h:6 * h + 6] = dJh
        out["dJv"][6 * h:6 * h + 6] = dJh @ v
    return out
