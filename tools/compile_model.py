"""Compile the reference scene's URDFs into the kernel's model tables.

    python tools/compile_model.py [/root/reference]

Writes `<pkg>/ikgrasp/data/nextage_dualarm.json`, `nextage_inertia.json`,
`nextage_actuation.json` and `nextage_collision.json` (committed: the GPU box has no reference tree).
Inputs: `models/nextagea_description/urdf/NextageaOpen.urdf` (kinematics, the
links' <inertial> entries and the joints' <limit velocity effort>) and `models/cubes/cube_small.urdf`
(config.py:44-51), base placement
ROBOT_PLACEMENT = (I, [0, 0, 0.85]) (config.py:33).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "motion-planning-and-control-for-dual-manipulator-robot_amd"))

from ikgrasp.collision import NEXTAGE_COLLISION_JSON, build_scene  # noqa: E402
from ikgrasp.model import (ActuatorLimits, BodyInertias, DualArmModel, NEXTAGE_ACTUATION_JSON,  # noqa: E402
                           NEXTAGE_INERTIA_JSON, NEXTAGE_JSON)
from ikgrasp.se3 import rotate  # noqa: E402


def main(ref="/root/reference"):
    robot = os.path.join(ref, "models/nextagea_description/urdf/NextageaOpen.urdf")
    cube = os.path.join(ref, "models/cubes/cube_small.urdf")
    base = (np.eye(3), np.array([0.0, 0.0, 0.85]))
    m = DualArmModel.from_urdf(robot, cube, base_placement=base)
    os.makedirs(os.path.dirname(NEXTAGE_JSON), exist_ok=True)
    with open(NEXTAGE_JSON, "w") as f:
        f.write(m.to_json())
    print(f"wrote {NEXTAGE_JSON}: nq={m.nq} root={m.root_q} arms={m.arm_q.tolist()}")
    # body inertias (control.py:284-286: M and b of pin.computeAllTerms / nonLinearEffects)
    bi = BodyInertias.from_urdf(robot).validate()
    with open(NEXTAGE_INERTIA_JSON, "w") as f:
        f.write(bi.to_json())
    print(f"wrote {NEXTAGE_INERTIA_JSON}: {bi.nq} bodies, {bi.mass.sum():.6g} kg")
    # what the motors can do (<limit velocity effort>): control.dyntraj / retime
    al = ActuatorLimits.from_urdf(robot)
    with open(NEXTAGE_ACTUATION_JSON, "w") as f:
        f.write(al.to_json())
    print(f"wrote {NEXTAGE_ACTUATION_JSON}: velocity {sorted(set(al.velocity.tolist()))} effort {sorted(set(al.effort.tolist()))}")
    # collision scene (setup_pinocchio.py:53-83; placements config.py:33-37)
    urdf = os.path.join(ref, "models/nextagea_description/urdf")
    scene = build_scene(
        os.path.join(urdf, "NextageaOpen.urdf"), os.path.join(urdf, "NextageAOpen.srdf"),
        os.path.join(ref, "models/table/table_tallerscaled.urdf"), os.path.join(ref, "models/cubes/obstacle.urdf"),
        cube, m.joint_names, base,
        (rotate("z", -np.pi / 2), np.array([0.8, 0.0, 0.0])),
        (rotate("z", 0.0), np.array([0.43, -0.1, 0.94])),
        (rotate("z", 0.0), np.array([0.33, -0.3, 0.93])), axis_frames=m.axis_frames())
    with open(NEXTAGE_COLLISION_JSON, "w") as f:
        f.write(scene.to_json())
    print(f"wrote {NEXTAGE_COLLISION_JSON}: {len(scene.geoms)} geometries, {len(scene.pairs)} pairs")


if __name__ == "__main__":
    main(*sys.argv[1:])
