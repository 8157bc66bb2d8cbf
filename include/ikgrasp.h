/*
 * ikgrasp — MI355X-native batched dual-arm grasp-pose inverse kinematics.
 *
 * C-ABI of libikgrasp.so (plain pointers and sizes; no C++ or torch types).
 * It replaces the per-call Pinocchio loop of the reference:
 *
 *   computeqgrasppose(robot, qcurrent, cube, cubetarget, viz=None)
 *       /root/reference/inverse_geometry.py:17-100
 *
 * whose Python->C++ crossings (pin.framesForwardKinematics :58,
 * pin.computeJointJacobians :59, pin.log :66-67, pin.computeFrameJacobian
 * :75-76, np.linalg.pinv :83, pin.integrate :86, projecttojointlimits :89 ->
 * tools.py:21-22) are fused into one HIP kernel launch over a batch.
 * The ctypes binding a maintainer adds on the reference side is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - SE(3) placements are 12 scalars: R row-major (9) then t (3).
 *   - Motion vectors are [linear; angular] (Pinocchio convention).
 *   - Float arrays use the dtype selected by `dtype` (IKG_F64 / IKG_F32).
 *   - All buffers are owned by the caller.  They are device pointers unless
 *     IKG_FLAG_HOST_POINTERS is set, in which case the library stages them
 *     through device scratch and synchronises the stream before returning.
 *   - Float inputs must be finite.  With IKG_FLAG_HOST_POINTERS the solve
 *     entry points check targets, q0 and seeds and return IKG_EINVAL for a
 *     NaN/inf; device-pointer callers own the check (the kernels are built
 *     with finite-math assumptions, so a non-finite input gives unspecified
 *     values for that problem's outputs).
 *   - Return 0 on success, a negative IKG_E* code on failure; the message of
 *     the last failure on the calling thread is ikg_last_error().  Nothing
 *     throws or exits across this boundary.
 *   - Calls are re-entrant per (model, stream).
 *   - Results are deterministic: no answer depends on the order in which a
 *     launch's waves run, on the batch size or on a problem's position, with
 *     the exceptions below.  With the collision term, a problem that
 *     converges into collision runs on in the batch kernel itself, which
 *     writes a checkpoint of its loop state per 32-update window into the
 *     problem's own fixed slot; the scan proves windows colliding with a
 *     certificate, and a window it cannot prove is regenerated from its
 *     checkpoint by the same loop compiled as the resume kernel.  Which path
 *     a problem takes is a function of that problem alone, so its answer is
 *     the same in any batch, chunking (a batch whose checkpoints exceed their
 *     budget, IKG_CK_BUDGET_MB, runs as equal launches in the whole batch's
 *     layout) or records round (IKG_REC_BUDGET_MB); the regenerated iterates
 *     agree with the batch loop's to rounding (the two instantiations
 *     contract a few products into FMAs differently: flags and update counts
 *     equal, q <= 1e-12 fp64 on the tests' batches).  Those kernels recompute
 *     the carried joint trig exactly at every window start (every 32 updates
 *     in fp64, 128 without the collision term), so a problem that never
 *     collides gets the same answer as without the term to rounding, not bit
 *     for bit.  (Models the batch
 *     kernel does not record for -- generic or run-time-compiled kernels,
 *     lambda > 0, the QUAD layout -- run on in the trajectory kernel, which
 *     agrees with the batch loop to rounding, q <= 1e-9.)  And in
 *     fp64 a broadcast q0
 *     (q0_stride = 0) and per-problem q0 rows (and multi-start seeds)
 *     advance the joint sin/cos by different rules for steps of
 *     0.025..0.25 rad (exact sincos / a longer series), so when such steps
 *     occur -- random seeds, not the reference's q0 = 0 on its sampler's
 *     targets -- the two agree to rounding (q <= 1e-10, end effectors
 *     <= 1e-12 over 150 updates), not bit for bit.  fp32 takes the longer
 *     series for every q0 layout: its answer does not depend on how q0 is
 *     passed.  A multi-start's seed equals a per-row solve of that seed bit
 *     for bit.  fp32 results also depend on the kernel layout (PAIR /
 *     PACKED), which AUTO picks by batch size.
 *
 * Graphs
 *   - Device-pointer solves are stream-ordered and may be captured into a
 *     hipGraph (no host synchronisation, no blocking allocation).  Scratch a
 *     captured solve needs (records, multi-start and continuation workspaces)
 *     is allocated at capture time and owned by the captured graph (a graph
 *     user object).  When the graph and all its executable instantiations
 *     are destroyed the buffer goes on the model's pending list: a later
 *     capture on the model reuses it if it is large enough (so recapturing
 *     every cycle holds a bounded number of buffers), and the model's next
 *     uncaptured solve, ikg_model_trim or ikg_model_destroy frees it.
 *   - All instantiations of one captured graph share that scratch: do not
 *     launch two of them concurrently (on different streams).
 *   - Destroy graphs before the model: they also reference its device tables.
 *
 * Scratch memory
 *   - Uncaptured solves take their scratch from a stream-ordered pool the
 *     model owns (one per device it solves on).  The pool keeps up to
 *     1.25 GiB of freed memory reserved for the next solve (environment
 *     IKG_WS_KEEP_MB overrides the amount) and releases the rest at the next
 *     synchronisation.  A collision solve holds, while it runs, its window
 *     checkpoints (17 KB per fp64 problem, 8.7 KB fp32, at max_iters 1,000)
 *     and the records of the problems its scan regenerates, up to the
 *     records budget (1 GiB).  ikg_model_trim synchronises each such device and
 *     releases everything the pools hold unused; ikg_model_destroy
 *     synchronises and destroys the pools.  Released memory goes back to the
 *     HIP runtime, which keeps it mapped for later pools and allocations of
 *     the process (the device's free-memory figure does not rise; a second
 *     model reuses it without taking more of the device), and a destroyed
 *     model leaves that figure where it was before the model existed
 *     (tests/test_gpu_memory.py).  IKG_WS_POOL=0 in the environment
 *     selects the device's default pool.
 */
#ifndef IKGRASP_H
#define IKGRASP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IKG_MAX_NQ 32
#define IKG_ARM_DOF 6
#define IKG_MAX_GEOMS 64
#define IKG_MAX_PAIRS 1024

enum ikg_dtype { IKG_F64 = 0, IKG_F32 = 1 };

enum ikg_status {
  IKG_OK = 0,
  IKG_EINVAL = -1,      /* bad argument / unsupported model structure */
  IKG_EHIP = -2,        /* HIP runtime error */
  IKG_ENOMEM = -3,      /* device allocation failed */
  IKG_ENODEV = -4       /* no such device */
};

/* flags */
#define IKG_FLAG_HOST_POINTERS 1u

/* kernel variant selector (ikg_params.variant) */
enum ikg_variant {
  IKG_VARIANT_AUTO = 0,   /* ikg_solve_batch: PACKED where it applies and B > 4 pair waves
                             per CU, else PAIR (QUAD measured no faster: explicit only);
                             ikg_solve_multistart: PAIR */
  IKG_VARIANT_PAIR = 1,   /* two lanes per problem (one arm per lane), 32 problems / wave */
  IKG_VARIANT_PACKED = 2, /* fp32, Nextage-class models, lambda = 0: one lane per problem with
                             both arms packed in 2-vectors (v_pk_*_f32), 64 problems / wave */
  IKG_VARIANT_QUAD = 3    /* Nextage-class models, lambda = 0: four lanes per arm (rows of the
                             kinematic chain split over them), 8 problems / wave */
};

/* Robot + grasp-object description (produced by the model compiler,
 * ikgrasp/model.py, from the URDFs — setup_pinocchio.py:73-83). */
typedef struct ikg_model_desc {
  int32_t nq;                        /* configuration size (15 for Nextage) */
  int32_t parent[IKG_MAX_NQ];        /* parent joint (q index), -1 = universe */
  int32_t axis[IKG_MAX_NQ];          /* 0/1/2 = revolute about +X/+Y/+Z */
  double placement[IKG_MAX_NQ][12];  /* joint placement in parent frame (R row-major, t) */
  double lower[IKG_MAX_NQ];          /* joint limits (projecttojointlimits, tools.py:21-22) */
  double upper[IKG_MAX_NQ];
  int32_t root_q;                    /* shared joint feeding both arms (chest) */
  int32_t arm_q[2][IKG_ARM_DOF];     /* left/right arm joints, proximal -> distal */
  double hand[2][12];                /* LARM_EFF / RARM_EFF frame in last arm joint frame */
  double hook[2][12];                /* LARM_HOOK / RARM_HOOK in the cube frame (cube_small.urdf:34-47) */
} ikg_model_desc;

/* Loop hyper-parameters; defaults equal the reference
 * (EPSILON config.py:22, DT and max_iters inverse_geometry.py:53-54). */
typedef struct ikg_params {
  double eps;          /* stop when |log6 err| < eps for both hands (1e-3) */
  double dt;           /* q <- clip(q + dt * dq) (1e-2) */
  int32_t max_iters;   /* joint updates before giving up (1000) */
  int32_t variant;     /* enum ikg_variant */
  double lambda;       /* damping of (J J^T + lambda I); 0 = pinv semantics (reference) */
  int32_t problems_per_wave; /* 1..32 problems per 64-lane wave; 0 = auto (32) */
  int32_t check_collision;   /* 1: reference `success` = converged AND collision-free, iterating on while
                                converged-but-colliding (inverse_geometry.py:70, :97-98); needs
                                ikg_model_set_collision.  0: convergence only (default). */
} ikg_params;

/* Collision scene (tools.py:25-35 collision(); pairs built in
 * setup_pinocchio.py:53-60), produced by ikgrasp/collision.py. */
enum ikg_geom_kind {
  IKG_GEOM_SPHERE = 0,    /* dims: radius */
  IKG_GEOM_BOX = 1,       /* dims: half extents */
  IKG_GEOM_CYLINDER = 2,  /* dims: radius, half length (local z) */
  IKG_GEOM_MESHBOX = 3    /* convex hull of a box mesh (the cube): half extents */
};
typedef struct ikg_collision_desc {
  int32_t n_geoms;
  int32_t kind[IKG_MAX_GEOMS];
  int32_t joint[IKG_MAX_GEOMS];          /* q index of the parent joint, -1 = world-fixed */
  double placement[IKG_MAX_GEOMS][12];   /* in the parent joint frame (world if joint = -1) */
  double dims[IKG_MAX_GEOMS][3];
  int32_t target_geom;                   /* geometry placed at each solve's cube target, -1 none */
  int32_t n_pairs;
  int32_t pairs[IKG_MAX_PAIRS][2];
} ikg_collision_desc;

typedef struct ikg_model ikg_model;

/* Build a device-ready model (tables are uploaded to every device lazily). */
int ikg_model_create(const ikg_model_desc* desc, ikg_model** out);
void ikg_model_destroy(ikg_model* model);

/* Return the scratch memory the model's pools keep for later solves (and the
 * buffers of destroyed captured graphs) to the driver; the model stays usable.
 * Synchronises every device the model has solved on.  No reference
 * counterpart (the reference allocates nothing on a device). */
int ikg_model_trim(ikg_model* model);

/* Attach (or replace) the collision scene of a model. */
int ikg_model_set_collision(ikg_model* model, const ikg_collision_desc* desc);

/*
 * Compile the pair-layout kernels against this model's tables (hipRTC, gfx950)
 * and use them for later ikg_solve_batch / ikg_solve_multistart calls of
 * `dtype` on `device` that run the pair layout (not PACKED / QUAD).  Joint
 * axes, identity placements, zero offsets and limits become compile-time
 * constants; results match the prebuilt kernels' (same flags and update
 * counts, q to rounding: folded exact 0 / 1 terms).  The first call per
 * model and dtype compiles (about 0.5 s), later devices only load.  `flags`: 0,
 * or IKG_SPECIALIZE_IF_GENERIC to do nothing (and return IKG_OK) for a model the
 * prebuilt library already specialises (Nextage class).  Do not call
 * concurrently with a solve on the same model.  With the environment variable
 * IKG_JIT_CACHE_DIR set, code objects are cached there (keyed by the generated
 * source, the embedded device headers and the compile options).  No reference
 * counterpart: inverse_geometry.py has one Python-level model
 * (setup_pinocchio.py:73-83); this is the per-model code generation the batched
 * library adds.
 */
#define IKG_SPECIALIZE_IF_GENERIC 1u
int ikg_model_specialize(ikg_model* model, int device, int dtype, uint32_t flags);
/* 1 if ikg_model_specialize succeeded for (device, dtype), else 0. */
int ikg_model_is_specialized(const ikg_model* model, int device, int dtype);

/* Fill `p` with the reference defaults. */
void ikg_params_default(ikg_params* p);

/*
 * Batched computeqgrasppose (inverse_geometry.py:17-100).  With
 * params->check_collision = 1 (needs ikg_model_set_collision) the stop test is
 * the reference's `errors pass and not collision(q)` (:70) and a final
 * colliding q is a failure (:97-98); with 0 it is the error test only.
 *   targets   [B,12]  cube placements (cubetarget); hooks are applied inside
 *   q0        [B,nq] (q0_stride = nq) or [nq] broadcast (q0_stride = 0)
 *   q_out     [B,nq]  first iterate with both errors < eps, else the iterate
 *                     after max_iters updates (same as the reference)
 *   converged [B]     1 if the stop test passed (the reference `success`
 *                     when check_collision = 1)
 *   iters     [B]     joint updates performed (may be NULL)
 *   err_out   [B,2]   |log6| of left/right hand at q_out (may be NULL)
 */
int ikg_solve_batch(const ikg_model* model, int device, int dtype,
                    const void* targets, const void* q0, int64_t q0_stride, int64_t B,
                    const ikg_params* params,
                    void* q_out, uint8_t* converged, int32_t* iters, void* err_out,
                    void* stream, uint32_t flags);

/*
 * Multi-start: every target is solved from every seed (S seeds x T targets);
 * per target the best seed is kept: lowest max(|eL|,|eR|) among converged
 * seeds, else lowest overall (ties -> lowest seed index).
 *   seeds [S,nq]; outputs per target: q_out [T,nq], converged [T], iters [T],
 *   err_out [T,2], best_seed [T] (any output but q_out may be NULL).
 */
int ikg_solve_multistart(const ikg_model* model, int device, int dtype,
                         const void* targets, int64_t T, const void* seeds, int64_t S,
                         const ikg_params* params,
                         void* q_out, uint8_t* converged, int32_t* iters, void* err_out,
                         int32_t* best_seed, void* stream, uint32_t flags);

/*
 * Batched effector forward kinematics (pin.framesForwardKinematics +
 * data.oMf[LARM_EFF/RARM_EFF], inverse_geometry.py:58-63).
 *   q [B,nq] -> hands [B,2,12]
 */
int ikg_fk_batch(const ikg_model* model, int device, int dtype,
                 const void* q, int64_t B, void* hands, void* stream, uint32_t flags);

/*
 * Batched SE(3) logarithm, pin.log6 (the pose error of
 * inverse_geometry.py:66-67): M [B,12] -> out [B,6] = [v; w].
 * fp64, for a rotation angle between 2^-13 and pi - 1e-2: w is within
 * eps / sin(theta) and v within eps |p| / sin^2(theta) of the exact value (the
 * acos angle's error, 1.4e-12 and 7.5e-9 |p| at 1.3e-4 rad); elsewhere and in
 * fp32 within the reference's own rounding.
 */
int ikg_log6_batch(int device, int dtype, const void* M, int64_t B, void* out, void* stream, uint32_t flags);

/*
 * Batched collision query, tools.collision(robot, q) (tools.py:25-35) with the
 * cube placed at each target (setcubeplacement, tools.py:62-68):
 *   q [B,nq], targets [B,12] -> in_collision [B] (1 = some active pair intersects)
 */
int ikg_collision_batch(const ikg_model* model, int device, int dtype, const void* q, const void* targets,
                        int64_t B, uint8_t* in_collision, void* stream, uint32_t flags);

/*
 * Batched distance query, tools.distanceToObstacle(robot, q) (tools.py:37-51):
 * the minimum over the active pairs listed in pair_idx (indices into the
 * scene's pair list; the reference takes the pairs whose second geometry is
 * the table or the obstacle) of the pair distance (hpp-fcl
 * computeDistance().min_distance; <= 0 when the pair intersects):
 *   q [B,nq], targets [B,12] -> dist [B].  pair_idx is a host array.
 */
int ikg_distance_batch(const ikg_model* model, int device, int dtype, const void* q, const void* targets,
                       int64_t B, const int32_t* pair_idx, int32_t n_pairs, void* dist, void* stream,
                       uint32_t flags);

/*
 * Batched cube-placement check of the planner's sampler / path projection
 * (path.py:51-52, :136-138: pin.computeCollisions on the cube's own collision
 * model, setup_pinocchio.py:62-70): the scene's target geometry placed at each
 * targets[i] against the world-fixed geometries listed in geoms (host array):
 *   targets [B,12] -> in_collision [B].
 */
int ikg_target_env_batch(const ikg_model* model, int device, int dtype, const void* targets, int64_t B,
                         const int32_t* geoms, int32_t n_geoms, uint8_t* in_collision, void* stream,
                         uint32_t flags);

/*
 * Controller kinematics: the kinematic terms of the
 * task-space controller, control.py:284-345, for a batch of states.
 * Replaces, per state and per hand (LARM_EFF, RARM_EFF):
 *   pin.computeAllTerms + updateFramePlacements -> data.oMf     (control.py:284-287, :305)
 *   pin.getFrameVelocity(model, data, fid, rf)                  (:310-313)
 *   pin.computeFrameJacobian(model, data, q, fid, rf)           (:341-342)
 *   pin.getFrameJacobianTimeVariation(model, data, fid, rf)     (:343-344)
 *   J_dot @ vq                                                  (:345)
 *   the desired-state FK (:292-294) and the PD errors (:314-333)
 * rf: enum ikg_reference_frame (the controller uses LOCAL_WORLD_ALIGNED).
 *   q, v [B,nq] (v may be NULL = zero velocity); q_des, v_des [B,nq] are only
 *   read for err/derr (v_des NULL = 0).  Every output is optional (NULL):
 *   placement [B,2,12]   oMf of LARM_EFF, RARM_EFF
 *   velocity  [B,2,6]    frame velocity in rf
 *   J, dJ     [B,12,nq]  rows 0-5 LARM_EFF, 6-11 RARM_EFF (np.vstack, :369), in rf;
 *                        dJ = d/dt J along q' = v
 *   dJv       [B,12]     dJ v
 *   err       [B,12]     per hand [x_des - x; log3(R_des R^T)]     (:326-327)
 *   derr      [B,12]     per hand v_des - v, LOCAL_WORLD_ALIGNED   (:330-331)
 */
enum ikg_reference_frame { IKG_WORLD = 0, IKG_LOCAL = 1, IKG_LOCAL_WORLD_ALIGNED = 2 };
typedef struct ikg_frame_kin_out {
  void* placement;
  void* velocity;
  void* J;
  void* dJ;
  void* dJv;
  void* err;
  void* derr;
} ikg_frame_kin_out;
int ikg_frame_kinematics_batch(const ikg_model* model, int device, int dtype, const void* q, const void* v,
                               const void* q_des, const void* v_des, int64_t B, int rf,
                               const ikg_frame_kin_out* out, void* stream, uint32_t flags);

/*
 * Controller dynamics: M and b of control.py:284-286 for a batch of states.
 * Replaces
 *   pin.computeAllTerms(model, data, q, vq); M = data.M      (control.py:284-285)
 *   b = pin.nonLinearEffects(model, data, q, vq)             (:286)
 * for any joint tree ikg_model_create accepts (passive joints may hang
 * anywhere).  The body inertias are attached with ikg_model_set_inertia: per
 * joint in q order the inertia of the body it moves -- its child link plus
 * every link fixed to it, as Pinocchio's URDF loader merges them -- in the
 * model's (canonical) joint frame.  mass >= 0; the inertia about the centre of
 * mass must be positive semi-definite with principal moments obeying the
 * triangle inequalities, else IKG_EINVAL.  gravity is in the world frame
 * (Pinocchio's model.gravity and setup_pybullet.py:33: (0, 0, -9.81)).
 *   q, v [B,nq] (v NULL = zero velocity).  Every output is optional (NULL):
 *   M    [B,nq,nq]  joint-space inertia matrix, both triangles filled
 *                   (data.M after computeAllTerms, symmetrised: the controller
 *                   inverts it and multiplies by it, :348, :401)
 *   nle  [B,nq]     pin.nonLinearEffects = C(q,v) v + g(q)
 *   g    [B,nq]     nle at zero velocity (pin.computeGeneralizedGravity)
 * Without attached inertias the call returns IKG_EINVAL.  Host-pointer calls
 * check q and v for finiteness; B == 0 is a no-op.  Stream-ordered, no
 * scratch memory, capturable like the other entries.
 */
typedef struct ikg_inertia_desc {
  double mass[IKG_MAX_NQ];
  double com[IKG_MAX_NQ][3];     /* in the (canonical) joint frame */
  double inertia[IKG_MAX_NQ][6]; /* xx xy xz yy yz zz about the com, joint-frame axes */
  double gravity[3];             /* world frame */
} ikg_inertia_desc;
int ikg_model_set_inertia(ikg_model* model, const ikg_inertia_desc* desc);

typedef struct ikg_dynamics_out {
  void* M;
  void* nle;
  void* g;
} ikg_dynamics_out;
int ikg_dynamics_batch(const ikg_model* model, int device, int dtype, const void* q, const void* v, int64_t B,
                       const ikg_dynamics_out* out, void* stream, uint32_t flags);

/*
 * The controller's torques: the second half of controllaw, control.py:284-406,
 * for a batch of states with no host round trip: the kinematic terms of
 * ikg_frame_kinematics_batch (LOCAL_WORLD_ALIGNED) and M, nle of
 * ikg_dynamics_batch go to device scratch from the model's workspace pool, then
 * one solve kernel does, per state and per hand h (rows 0-5 LARM_EFF, 6-11 RARM_EFF):
 *   Lambda_h = (J_h M^-1 J_h^T + lambda_reg 1)^-1                        (:348-349)
 *   fc_h = [Kf e_t; Kt e_r];  xdd_h = Kp e + Kv e' + Lambda_h fc_h      (:338-360)
 *   qdd = (J^T J + qp_reg 1)^-1 J^T (xdd - dJ v)                        (:381-395)
 *     quadprog.solve_qp(H, d) without constraints minimises 1/2 x^T H x - d^T x,
 *     i.e. x = H^-1 d with d = -J^T (dJ v - xdd) after the reference's d_qp = -d_qp
 *   tau = M qdd + nle + J^T (fc + fc_bias); tau[j] = 0 for j in zero_tau_mask  (:375, :401-406)
 * Each inverse is a Cholesky-type (L D L^T) factorisation of a symmetric
 * positive definite matrix.  The reference's try/except -> zeros (:396-398)
 * cannot trigger for such an H; should a pivot of H come out non-positive
 * (non-finite input only), qdd is written as zeros as the reference would.
 * fp64 ONLY: the 1e-6 regularisation of the rank-deficient nq x nq system
 * (the head columns of J are zero) leaves fp32 no correct digits.
 *   q, v, q_des, v_des [B,nq] (v, v_des NULL = zero).  Outputs, all optional:
 *   tau    [B,nq]    what sim.step receives (:410)
 *   qdd    [B,nq]    the QP's solution (exactly 0 where J^T(...) is exactly 0: the head joints)
 *   xdd    [B,12]    x_ddot_des_total (:371)
 *   Lambda [B,2,36]  per hand, row-major 6 x 6
 *   fc     [B,12]    f_c_total BEFORE the bias (the bias enters tau only, :375, :401)
 * Needs ikg_model_set_inertia (else IKG_EINVAL).  Host-pointer calls check the
 * inputs for finiteness.  B == 0 is a no-op.  Stream-ordered and capturable
 * like the other entries (scratch: "Graphs" above).
 */
typedef struct ikg_control_params { /* defaults = control.py:248-251, :349, :375, :386, :404 */
  double Kp, Kv, Kf, Kt;            /* 7000, 2 sqrt(Kp), 30, 2 sqrt(Kf) */
  double lambda_reg, qp_reg;        /* 1e-6, 1e-6 */
  double fc_bias[12];               /* zeros except [1] = -200 */
  uint32_t zero_tau_mask;           /* bits 1 and 2 */
} ikg_control_params;
void ikg_control_params_default(ikg_control_params* p);

typedef struct ikg_control_out {
  void* tau;
  void* qdd;
  void* xdd;
  void* Lambda;
  void* fc;
} ikg_control_out;
int ikg_control_torque_batch(const ikg_model* model, int device, const void* q, const void* v, const void* q_des,
                             const void* v_des, int64_t B, const ikg_control_params* params,
                             const ikg_control_out* out, void* stream, uint32_t flags);

/*
 * Forward dynamics: qdd = M(q)^-1 (tau - nle(q, v)), i.e. pin.aba(model, data,
 * q, v, tau), for a batch of states (fp64).  The dynamics kernel writes nle to
 * device scratch from the model's workspace pool (65,536 states per pass); a
 * second kernel forms M in LDS, each row about its own joint's origin so that
 * the small rows keep their relative accuracy under the division, factors
 * M = L D L^T and substitutes.
 *   q, v, tau [B,nq] (v NULL = zero velocity);  qdd [B,nq].
 * Needs ikg_model_set_inertia (else IKG_EINVAL).  Host-pointer calls check the
 * inputs for finiteness.  B == 0 is a no-op.  Stream-ordered and capturable
 * like ikg_control_torque_batch.
 */
int ikg_forward_dynamics_batch(const ikg_model* model, int device, const void* q, const void* v, const void* tau,
                               int64_t B, void* qdd, void* stream, uint32_t flags);

/*
 * A Bezier curve with the semantics of the reference's Bezier.__call__ /
 * eval_horner (control.py:30-46): out[k] = curve(times[k]) for K times (fp64).
 *   points [n_points, dim] is always a HOST array (it travels as kernel
 *   arguments); times [K] and out [K, dim] are device arrays, or host arrays
 *   with IKG_FLAG_HOST_POINTERS.
 * A curve of two control points returns mult * P0 whatever the time, as the
 * reference does.  n_points < 2, n_points > 64, dim outside [1, IKG_MAX_NQ] or
 * t_max <= t_min return IKG_EINVAL.  With host pointers a time outside
 * [t_min, t_max] returns IKG_EINVAL (the reference raises there); device-pointer
 * callers keep their times in range.  K == 0 is a no-op.
 */
int ikg_bezier_eval_batch(int device, const double* points, int32_t n_points, int32_t dim, double t_min, double t_max,
                          double mult, const void* times, int64_t K, void* out, void* stream, uint32_t flags);

/*
 * Closed-loop rollout: B copies of the reference's demo loop (control.py:461-463)
 * with a rigid-body plant in place of the simulator, `ticks` ticks in one call
 * and no host round trip between them.  A tick k of a state (q, v, t):
 *   1. q_des = Bq(clamp(t)), v_des = Bv(clamp(t)): each curve evaluated at t
 *      clamped to its own [t_min, t_max] (the reference's loop never leaves the
 *      range; clamping holds the end point)
 *   2. tau = the torque law of ikg_control_torque_batch (control.py:284-406)
 *   3. qdd = M^-1 (tau - nle)
 *   4. v += dt_sim qdd, then q += dt_sim v   (semi-implicit Euler, Bullet's scheme)
 *   5. t += dt_traj                          (one fp64 add, as `tcur += DT`)
 * dt_traj defaults to 1e-2 with dt_sim = 1e-3 (config.py:21): the reference
 * advances its trajectory clock by DT = 0.01 per 1 ms simulator tick
 * (control.py:449, :463), and the default keeps that.
 * THE PLANT is the free rigid-body tree of ikg_model_set_inertia: no contact, no
 * cube, no joint limits and no joint damping.  The default fc_bias (-200 N,
 * control.py:375) therefore has nothing to push against here: it accelerates
 * the arms; pass fc_bias = 0 for a free-space tracking run.
 * Per tick three kernels run (frame kinematics, dynamics, step); batches above
 * 65,536 states run chunk by chunk, all ticks of a chunk before the next chunk.
 *   q0, v0 [B,nq] (v0 NULL = zero) are never written and must not overlap the
 *   outputs; t0 [B] or NULL = the q curve's t_min.  q_curve and v_curve have
 *   dim = nq (ikg_bezier.points is a host array whatever the flags); a curve of
 *   a derivative carries its own mult (Bezier.derivative: mult / (t_max - t_min)).
 *   Outputs, all optional: the final q, v [B,nq] and t [B]; with record_every > 0
 *   q_hist, v_hist, tau_hist [B,R,nq], R = ticks / record_every: record j is
 *   the state after tick (j + 1) record_every - 1 and the tau applied in that tick.
 * fp64 only, like the torque law.  Needs ikg_model_set_inertia.  Host-pointer
 * calls check q0, v0, t0 for finiteness.  B == 0 is a no-op.  Stream-ordered and
 * capturable with device pointers (scratch: "Graphs" above).
 */
typedef struct ikg_bezier {
  const double* points; /* host, [n_points, nq] */
  int32_t n_points;     /* 2 .. 64 */
  double t_min, t_max;
  double mult;
} ikg_bezier;

typedef struct ikg_rollout_params {
  ikg_control_params control;
  double dt_sim;        /* 1e-3 */
  double dt_traj;       /* 1e-2 */
  int32_t ticks;        /* >= 0 */
  int32_t record_every; /* 0 = no history */
} ikg_rollout_params;
void ikg_rollout_params_default(ikg_rollout_params* p);

typedef struct ikg_rollout_out {
  void* q;
  void* v;
  void* t;
  void* q_hist;
  void* v_hist;
  void* tau_hist;
} ikg_rollout_out;
int ikg_control_rollout(const ikg_model* model, int device, const void* q0, const void* v0, const void* t0, int64_t B,
                        const ikg_bezier* q_curve, const ikg_bezier* v_curve, const ikg_rollout_params* params,
                        const ikg_rollout_out* out, void* stream, uint32_t flags);

/*
 * ikg_control_rollout with one curve pair PER STATE: state p follows
 * q_curves->points[p] and v_curves->points[p].  Everything else is the entry
 * above tick for tick (clamping, torque law, plant, Euler step, records,
 * 65,536-state chunks -- the curves chunk with their states -- and graph
 * capture): the same kernels read each state's control points through a
 * per-state stride (stride 0 = the shared pair of ikg_control_rollout), so B
 * equal curves give the shared entry's result bit for bit.
 *   points [B, n_points, nq]: device array, or host with IKG_FLAG_HOST_POINTERS
 *   (then checked for finiteness); it is read during the ticks and must not
 *   overlap an output.  n_points, the range and mult are common to all states
 *   (n_points 2 .. 64, t_max > t_min); t0 NULL = the q curves' t_min.
 */
typedef struct ikg_bezier_set {
  const void* points; /* [B, n_points, nq], device or host per flag */
  int32_t n_points;
  double t_min, t_max, mult;
} ikg_bezier_set;
int ikg_control_rollout_curves(const ikg_model* model, int device, const void* q0, const void* v0, const void* t0,
                               int64_t B, const ikg_bezier_set* q_curves, const ikg_bezier_set* v_curves,
                               const ikg_rollout_params* params, const ikg_rollout_out* out, void* stream,
                               uint32_t flags);

/*
 * Batched Bezier trajectory fit: the reference's maketraj (control.py:63-197)
 * for B paths in one launch (fp64).  The reference runs SLSQP over all
 * (degree + 1) x dim control points under six equality constraints (end
 * positions, zero end velocities and accelerations).  Those pin
 *   P[0] = P[1] = P[2] = q0,   P[degree-2] = P[degree-1] = P[degree] = q1,
 * and what is left is linear least squares in the degree - 5 free points, per
 * joint: with X0 = linspace(q0, q1, degree + 1), the reference's initial guess,
 *   min_delta | A_f (X0_f + delta) + c - Y |^2 + ridge |delta|^2,
 *   A_f[k,i] = C(degree,i) u_k^i (1 - u_k)^(degree-i), i = 3 .. degree-3,
 * c the pinned points' share, u_k = t_k / total_time with t = numpy's
 * linspace(0, total_time, n) (t_k = k (total_time / (n - 1)), t_{n-1} = total_time).
 * It is solved by a Householder factorisation of [A_f; sqrt(ridge) 1] (the normal
 * equations lose the control points: cond(A_f) ~ 2e5 at degree 20).  With
 * ridge = 0 and n >= degree - 3 this is the reference's problem and the result
 * its exact minimiser; ridge > 0 picks, for shorter paths, the solution nearest
 * X0 and damps the control polygon on noisy paths.
 *   q0, q1 [B,dim]; path_points packed [offsets[B],dim], path p = rows
 *   offsets[p] .. offsets[p+1]-1 (offsets [B+1], offsets[0] = 0; y_0 need not be q0).
 *   points  [B,degree+1,dim]  P[0..2] = q0 and P[degree-2..degree] = q1 are copies
 *   vpoints [B,degree,dim], apoints [B,degree-1,dim] (optional): the unscaled
 *           derivative control points as Bezier.derivative forms them,
 *           degree (P[i+1] - P[i]) and again; the 1 / total_time factors stay
 *           with the caller (ikg_bezier.mult)
 *   cost    [B]  sum_k |B(t_k) - y_k|^2 with the reference's Horner (result.fun)
 *   status  [B]  0 = solved, 1 = the path's point count is out of range
 * Limits: degree 6 .. 20, dim 1 .. IKG_MAX_NQ, 2 <= n <= 256 per path and
 * n >= degree - 3 unless ridge > 0, total_time > 0, ridge >= 0.  All arrays,
 * offsets included, are device arrays, or host arrays with
 * IKG_FLAG_HOST_POINTERS; a host-pointer call checks every limit and the inputs'
 * finiteness and returns IKG_EINVAL before any launch.  With device pointers the
 * kernel refuses a path whose count is out of range: status 1, cost NaN, its
 * points untouched, its neighbours unaffected.  B == 0 is a no-op.
 * Stream-ordered, no scratch, capturable.
 */
typedef struct ikg_fit_params {
  int32_t degree;    /* 20 (control.py:85) */
  double ridge;      /* 0 */
  double total_time; /* 1 */
} ikg_fit_params;
void ikg_fit_params_default(ikg_fit_params* p);
int ikg_bezier_fit_batch(int device, const void* q0, const void* q1, const void* path_points, const int64_t* offsets,
                         int64_t B, int32_t dim, const ikg_fit_params* params, void* points, void* vpoints,
                         void* apoints, void* cost, int32_t* status, void* stream, uint32_t flags);

/* ---- RRT-Connect planner primitives (path.py:125-278) ----
 * fp64 only (the planner's IK is fp64).  All arrays are device arrays, or host
 * arrays with IKG_FLAG_HOST_POINTERS (staged, checked for finiteness, the call
 * returns after the results are back).  With device pointers the calls are
 * stream-ordered and return without waiting.
 *
 * ikg_se3_interpolate_batch: pin.SE3.Interpolate for C placement pairs,
 *   out[c] = A[c] * exp6(alpha[c] * log6(A[c]^-1 B[c])),  A, B, out [C,12], alpha [C]
 * with Pinocchio's branches (log6 as ikg_log6_batch; exp6's Taylor series below
 * eps^(1/4)).  Rotations of A^-1 B within 0.01 rad of pi are not pinned.
 *
 * ikg_nearest_batch: the nearest node of P trees.  Tree p is the rows
 * nodes[p * cap .. p * cap + counts[p] - 1], each of length nq; rows at and
 * past counts[p] are never read as candidates.  index[p] is the row with the
 * least Euclidean distance to queries[p] (the squared distance summed over
 * j = 0 .. nq-1 in that order), the LOWEST index among exact ties; dist[p] the
 * square root of that sum.  counts[p] == 0 gives index -1 (dist 0).  A
 * host-pointer call rejects counts outside [0, cap]; with device pointers a
 * count above cap is read as cap.
 *   nodes [P,cap,nq], counts [P] int32, queries [P,nq], index [P] int32, dist [P]
 *
 * ikg_project_paths: path.py:125-163 (project_path) for C chains advanced in
 * lock-step.  Chain c interpolates cube_curr[c] -> cube_rand[c] in
 * steps = int(|dt| / step_size) + 1 steps; at step s it places the cube at
 * Interpolate(s / steps), checks the scene's target geometry there against the
 * listed world-fixed geometries (the narrow phase of ikg_target_env_batch),
 * solves the IK warm-started from its last accepted q (ikg_solve_batch with
 * `params`; the planner sets check_collision = 1) and appends (q, placement)
 * when the placement is free and the solve converged; otherwise the chain stops.
 *   q_curr [C,nq], cube_curr, cube_rand [C,12], geoms [n_geoms] (HOST array)
 *   robot_path [C,max_nodes,nq], cube_path [C,max_nodes,12]: row 0 is q_curr /
 *     cube_curr, rows 1 .. n_nodes[c]-1 the accepted steps; later rows are
 *     unspecified (zero with host pointers)
 *   n_nodes [C] int32, status [C] int32:
 *     0 reached cube_rand, 1 stopped by a placement collision, 2 stopped by a
 *     failed IK, 3 cut at max_nodes (status holds -1 while a chain advances)
 *   A chain that fills its last row at the step that reaches cube_rand is
 *   reached (0), not cut.  Otherwise status 3 wins over a stop that the next
 *   step would have produced: a chain whose n_nodes reaches max_nodes is cut
 *   there, whatever its next placement or solve would have given; max_nodes = 1
 *   cuts every chain at row 0.  The step count comes from the translations
 *   alone: a pure rotation (equal translations) is one step whatever its angle.
 * Per step a prepare kernel, the solve and a commit kernel are enqueued on
 * `stream`; nothing waits on the host.  A host-pointer call enqueues as many
 * steps as its longest chain needs, a device-pointer call max_nodes - 1.  The
 * scratch is stream-ordered (the model's pool).  Not capturable.  Needs
 * ikg_model_set_collision with a target geometry.  C == 0 is a no-op.
 */
int ikg_se3_interpolate_batch(int device, const void* A, const void* B, const void* alpha, int64_t C, void* out,
                              void* stream, uint32_t flags);
int ikg_nearest_batch(int device, const void* nodes, int64_t cap, const int32_t* counts, const void* queries,
                      int32_t nq, int64_t P, int32_t* index, void* dist, void* stream, uint32_t flags);
int ikg_project_paths(const ikg_model* model, int device, const void* q_curr, const void* cube_curr,
                      const void* cube_rand, int64_t C, double step_size, int32_t max_nodes, const int32_t* geoms,
                      int32_t n_geoms, const ikg_params* params, void* robot_path, void* cube_path, int32_t* n_nodes,
                      int32_t* status, void* stream, uint32_t flags);

/* ---- Trajectory check: collision, clearance, grasp and joint limits along curves ----
 * ikg_trajectory_check_batch samples each of B joint-space Bezier curves at S
 * times and answers, per sample and folded per curve, what the planner checks
 * at its vertices only.  fp64.  Per (curve b, sample k):
 *   t_k   = t_min + k (t_max - t_min) / (S - 1), t_{S-1} = t_max exactly
 *   q     = the curve at t_k (ikg_bezier_eval_batch's function: two control
 *           points give mult * P0 at every time)
 *   cube  = IKG_CUBE_CARRIED: oM(left effector) * hook_left^-1, the placement at
 *           which the left hand's IK error is zero; IKG_CUBE_FIXED: cube_fixed[b]
 *   grasp = norm(log6(oMhand^-1 * cube * hook)), the quantity the IK compares
 *           with eps: the right hand's (CARRIED; the left is zero by construction)
 *           or the larger of the two hands' (FIXED)
 *   limit = max(0, max_j(q_j - upper_j), max_j(lower_j - q_j)) (tools.jointlimitscost)
 *   collision = ikg_collision_batch's answer at (q, cube)
 *   clearance = ikg_distance_batch's answer at (q, cube) over pair_idx; computed
 *           only when n_pairs > 0 and a clearance output is requested, else the
 *           clearance outputs hold 1e30 and arg_clearance -1
 * Per curve: first_collision (lowest colliding sample, -1 none), first_pair (the
 * lowest-index colliding scene pair at that sample), n_collision, and the
 * minimum clearance / maximum grasp / maximum limit with the LOWEST sample among
 * exact ties.  Every output is optional (NULL).  The per-curve outputs are a
 * fold of the per-sample values in sample order; no output depends on
 * samples_per_wave.
 *   q_curves->points [B, n_points, nq], cube_fixed [B,12] (FIXED), the outputs:
 *     device arrays, or host arrays with IKG_FLAG_HOST_POINTERS
 *   pair_idx [n_pairs]: HOST array of scene pair indices (as ikg_distance_batch); may be
 *     NULL with n_pairs == 0
 * One 64-lane wave walks samples_per_wave consecutive samples of one curve and
 * carries the collision witness from one to the next; a second kernel folds the
 * waves' partial results per curve.  samples_per_wave == 0: the least run that
 * still gives about 2,048 waves (two rounds of one wave per SIMD), at most S.
 * A host-pointer call checks finiteness and every limit (S >= 2, n_points 2 .. 64,
 * t_max > t_min, cube_mode, FIXED with cube_fixed, pair_idx inside the scene's
 * pairs) and returns IKG_EINVAL before any launch; the limits are checked with
 * device pointers too.  Needs ikg_model_set_collision with a target geometry.
 * B == 0 is a no-op.  Stream-ordered; the scratch comes from the model's pool and
 * the call waits for the stream before it returns (the staged pair list is freed
 * on return).  Not capturable.
 */
#define IKG_CUBE_CARRIED 0
#define IKG_CUBE_FIXED 1
typedef struct ikg_trajcheck_params {
  int32_t samples;          /* S >= 2; 151 */
  int32_t cube_mode;        /* IKG_CUBE_CARRIED */
  int32_t samples_per_wave; /* 0 = chosen by the launcher; >= 1 forces it (tests) */
} ikg_trajcheck_params;
typedef struct ikg_trajcheck_out { /* every field optional (NULL) */
  int32_t* first_collision;        /* [B] lowest colliding sample, -1 = none */
  int32_t* first_pair;             /* [B] lowest-index colliding pair at that sample, -1 = none */
  int32_t* n_collision;            /* [B] colliding samples */
  void* min_clearance;
  int32_t* arg_clearance; /* [B] */
  void* max_grasp;
  int32_t* arg_grasp; /* [B] */
  void* max_limit;
  int32_t* arg_limit; /* [B] */
  uint8_t* collision; /* [B,S] */
  void* clearance;    /* [B,S] */
  void* grasp;        /* [B,S] */
  void* limit;        /* [B,S] */
  void* cube;         /* [B,S,12] the cube placement used at each sample */
} ikg_trajcheck_out;
void ikg_trajcheck_params_default(ikg_trajcheck_params* p);
/* what samples_per_wave == 0 resolves to for B >= 1 curves of `samples` >= 2 samples (0 otherwise) */
int ikg_trajcheck_samples_per_wave(int64_t B, int32_t samples);
int ikg_trajectory_check_batch(const ikg_model* model, int device, const ikg_bezier_set* q_curves, int64_t B,
                               const void* cube_fixed, const int32_t* pair_idx, int32_t n_pairs,
                               const ikg_trajcheck_params* params, const ikg_trajcheck_out* out, void* stream,
                               uint32_t flags);

/* ---- Trajectory dynamics: inverse dynamics and actuator limits along curves ----
 * ikg_trajectory_dynamics_batch samples each of B joint-space Bezier curves at
 * the S times of ikg_trajectory_check_batch and answers whether the motors can
 * follow the curve in T = t_max - t_min, and if not how long it must take.
 * fp64; M is never formed.  Per (curve b, sample k, joint j):
 *   t_k = t_min + k T / (S - 1), t_{S-1} = t_max exactly
 *   q   = the curve at t_k (ikg_bezier_eval_batch's function)
 *   v   = the same function of the derivative points n (P[i+1] - P[i]), n the
 *         degree, with multiplier mult * (1 / T); a = the same again from the v
 *         points, multiplier mult * (1 / T) * (1 / T) (Bezier.derivative(1), (2);
 *         every difference and product rounded, no fused multiply-add)
 *   tau = rnea(q, v, a), g = rnea(q, 0, 0) (recursive Newton-Euler, the body
 *         inertias and gravity of ikg_model_set_inertia), d = tau - g
 * Under a uniform time scaling t -> s t the curve keeps its points, v scales as
 * 1 / s and d as 1 / s^2, so the least feasible duration is a closed form of the
 * samples.  Per curve, with velocity_limit vlim_j and effort_limit E_j:
 *   speed_scale  = max |v| / vlim                     arg_speed
 *   torque_use   = max |tau| / E at the curve's own T arg_torque_use
 *   static_use   = max |g| / E                        arg_static
 *   n_static     = entries with |g| >= E: no duration helps these
 *   torque_scale = max over the other entries of sqrt(|d| / (E - sign(d) g)),
 *                  0 where d = 0                      arg_torque_scale
 * A duration s T meets every limit iff n_static == 0 and
 * s >= max(speed_scale, torque_scale).  A joint whose limit is IKG_NO_LIMIT
 * contributes 0.  Each arg output is [B,2] = (sample, joint) of the maximum;
 * among exact ties the lowest sample, then the lowest joint; (-1, -1) and a
 * value of 0 where no entry took part (torque_scale with every entry static).
 * Per sample, on request: tau, g [B,S,nq].  Every output is optional (NULL).
 *   q_curves->points [B, n_points, nq] and the outputs: device arrays, or host
 *     arrays with IKG_FLAG_HOST_POINTERS; the limits travel in params
 * A sample occupies 16 lanes (nq <= 16) or 32, one lane per body; one 64-lane
 * wave walks samples_per_wave consecutive samples of one curve, 4 or 2 side by
 * side, and a second kernel folds the waves' partial results per curve.  No
 * output depends on samples_per_wave (0: whole lane groups, about 8,192 waves).
 * n_points 5 .. 64 (below degree 4 the acceleration curve has two control
 * points, which the reference's Bezier evaluates as a constant), S >= 2,
 * t_max > t_min, every limit > 0.  A host-pointer call checks these and the
 * finiteness of its inputs and returns IKG_EINVAL before any launch; the limits
 * are checked with device pointers too.  Needs ikg_model_set_inertia.  B == 0 is
 * a no-op.  Stream-ordered; the scratch comes from the model's pool.  Not
 * capturable.
 */
#define IKG_NO_LIMIT 1e30
typedef struct ikg_trajdyn_params {
  int32_t samples;                   /* S >= 2; 151 */
  int32_t samples_per_wave;          /* 0 = chosen by the launcher; >= 1 forces it (tests) */
  double velocity_limit[IKG_MAX_NQ]; /* > 0; IKG_NO_LIMIT = unlimited */
  double effort_limit[IKG_MAX_NQ];
} ikg_trajdyn_params;
typedef struct ikg_trajdyn_out { /* every field optional (NULL) */
  void* speed_scale;             /* [B] */
  int32_t* arg_speed;            /* [B,2] (sample, joint) */
  void* torque_use;
  int32_t* arg_torque_use;
  void* static_use;
  int32_t* arg_static;
  int32_t* n_static; /* [B] */
  void* torque_scale;
  int32_t* arg_torque_scale;
  void* tau; /* [B,S,nq] */
  void* g;   /* [B,S,nq] */
} ikg_trajdyn_out;
void ikg_trajdyn_params_default(ikg_trajdyn_params* p); /* 151, 0, every limit IKG_NO_LIMIT */
int ikg_trajectory_dynamics_batch(const ikg_model* model, int device, const ikg_bezier_set* q_curves, int64_t B,
                                  const ikg_trajdyn_params* params, const ikg_trajdyn_out* out, void* stream,
                                  uint32_t flags);

/* Thread-local message of the last failure ("" if none). */
const char* ikg_last_error(void);

/* Library version string. */
const char* ikg_version(void);

#ifdef __cplusplus
}
#endif

#endif /* IKGRASP_H */
