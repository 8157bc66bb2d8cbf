"""Models, states and fixture access of the dynamics / controller family legs
(tests/test_dynamics_family.py, tests/test_gpu_dynamics_family.py; fixture
tests/golden/dynamics_family_cases.npz from make_dynamics_family_golden.py).

The kernels of csrc/ikg_dynamics.hip give a state G lanes (16 for nq <= 16,
else 32); what the lanes add to the arithmetic -- the parent fetch across a
group, idle lanes, the ancestor bit tests, the LDS tile of M and its two
store branches -- only shows on trees of different width, depth and order:

    model          nq  G   longest chain   what it adds
    nx_scaled      13  16   7   no passive joint, three idle lanes
    nx_extra_zero  16  16   7   every lane of a group is a body
    nx_zbreak, nx_rot, offset_wrist, wrist_edge, hand_general, hand_cross
                   15  16   7   rpy on joints and on the root, general hand frames
    mixed_17       17  32   7   the first G = 32 model: 15 idle lanes, odd nq
    mixed_axes     32  32  11   every lane a body; rotated base, unaligned and negative
                                axes, right arm first, passive chains before / between / after
    mixed_deep     32  32  17   a passive chain of ten below the last joint of an arm: the
                                `levels` loop runs past 16, parents in lanes 22..30

The nine committed members come from tests/golden/family; mixed_17 and
mixed_deep are built here and committed nowhere.
"""
import copy
import os
import tempfile

import numpy as np

import dynamics_oracle as do
import robot_family as rf

GOLDEN = rf.GOLDEN
FIXTURE = os.path.join(GOLDEN, "dynamics_family_cases.npz")

# one seed per model: dynamics_oracle.seeded_inertias(nq, seed); the states use STATE_SEED + seed
SEEDS = {"nx_scaled": 21, "nx_extra_zero": 22, "nx_zbreak": 23, "nx_rot": 24, "offset_wrist": 25, "wrist_edge": 26,
         "hand_general": 27, "hand_cross": 28, "mixed_axes": 29, "mixed_17": 30, "mixed_deep": 31}
STATE_SEED = 4000
NAMES = tuple(SEEDS)
N_STATES = 8
DYN = ("M", "nle", "g")
CTL = ("tau", "qdd", "xdd", "Lambda", "fc")
# scalar entries stored as one vector per kind: <kind>_<key> for key in the tuple
PACKED = {"err_f64": CTL, "tol": CTL, "fp32_err": DYN, "tol32": DYN}
DEEP_CHAIN = "AA_JOINT"  # the ten-joint passive chain of mixed_axes that mixed_deep hangs below an arm


def mixed_17_model():
    """mixed_axes without its AA_JOINT and M_JOINT chains: 1 + 6 + 6 + 4 joints.
    The grasp object is mixed_axes': the arms hang off the same chest link."""
    from ikgrasp.model import DualArmModel
    row = copy.deepcopy(rf.MEMBERS["mixed_axes"])
    row["passive"] = [c for c in row["passive"] if c[0] not in ("AA_JOINT", "M_JOINT")]
    with tempfile.TemporaryDirectory() as d:
        robot, cube = os.path.join(d, "mixed_17.urdf"), os.path.join(d, "mixed_17_cube.urdf")
        with open(robot, "w") as f:
            f.write(rf.robot_urdf("mixed_17", row))
        with open(cube, "w") as f:
            f.write(rf.cube_urdf("mixed_axes"))
        return DualArmModel.from_urdf(robot, cube, rf.base_placement("mixed_17", row))


def first_arm(model):
    """The arm (row of arm_q) that comes first in q order."""
    return int(np.argmin(model.arm_q[:, 0]))


def deep_chain(model):
    """q indices of mixed_axes' AA_JOINT chain, head first."""
    return [model.joint_names.index(f"{DEEP_CHAIN}{k}") for k in range(10)]


def mixed_deep_model():
    """(model, perm): mixed_axes with the head of its ten-joint AA_JOINT chain
    below the last joint of the arm that comes first in q order."""
    base = rf.load_model("mixed_axes")
    return do.hanging_passive_model(base, chain=deep_chain(base), below=base.arm_q[first_arm(base)][-1])


_MODELS = {}


def models():
    """{name: (DualArmModel, BodyInertias)}"""
    if not _MODELS:
        for name in NAMES:
            m = (mixed_17_model() if name == "mixed_17" else mixed_deep_model()[0] if name == "mixed_deep"
                 else rf.load_model(name))
            _MODELS[name] = (m, do.seeded_inertias(m.nq, SEEDS[name]))
    return _MODELS


def states(name, model, n=N_STATES):
    """q, v, q_des, v_des [n, nq]: q uniform within the limits clipped to +-2,
    v ~ N(0, 0.7), q_des = clip(q + N(0, 0.02)) to the limits, v_des = v + N(0, 0.1)."""
    rng = np.random.default_rng(STATE_SEED + SEEDS[name])
    nq = model.nq
    q = rng.uniform(np.maximum(model.lower, -2.0), np.minimum(model.upper, 2.0), (n, nq))
    v = rng.normal(0.0, 0.7, (n, nq))
    q_des = np.clip(q + rng.normal(0.0, 0.02, (n, nq)), model.lower, model.upper)
    v_des = v + rng.normal(0.0, 0.1, (n, nq))
    return q, v, q_des, v_des


def group_lanes(nq):
    """G of csrc/ikg_dynamics.hip launch_per_state."""
    return 16 if nq <= 16 else 32


def depths(parents):
    d = []
    for j, p in enumerate(parents):
        assert p < j
        d.append(1 if p < 0 else d[p] + 1)
    return d


def longest_chain(parents):
    return max(depths(parents))


def related(parents):
    """[nq, nq] bool: i == j, or one of i, j is an ancestor of the other.  M is
    exactly zero everywhere else."""
    n = len(parents)
    r = np.zeros((n, n), dtype=bool)
    for i in range(n):
        j = i
        while j >= 0:
            r[i, j] = r[j, i] = True
            j = parents[j]
    return r


def load_cases():
    """dynamics_family_cases.npz as {model: {key: array}} plus the pooled entries under ''."""
    d = dict(np.load(FIXTURE))
    out = {n: {} for n in NAMES}
    out[""] = {}
    for k, v in d.items():
        n = next((n for n in sorted(NAMES, key=len, reverse=True) if k.startswith(n + ".")), "")
        out[n][k[len(n) + 1:] if n else k] = v
    for c in out.values():
        for kind, keys in PACKED.items():
            if kind in c:
                c.update({f"{kind}_{k}": float(x) for k, x in zip(keys, c.pop(kind))})
    return out
