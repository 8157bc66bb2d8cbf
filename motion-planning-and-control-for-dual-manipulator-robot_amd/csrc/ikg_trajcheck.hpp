// Trajectory check (ikg_trajectory_check_batch): what one sample of one curve
// computes besides the collision check and the obstacle distance, and how the
// samples of a curve are folded into its verdict.  The functions are IKG_HD so
// the host emulator (ikg_host_emu.hip) runs the same arithmetic on the CPU; the
// wave kernel is in ikg_collision.hip, beside the checks it calls.
#pragma once

#include "ikg_collision.hpp"
#include "ikg_device.hpp"
#include "ikg_dynamics.hpp"

namespace ikg {

constexpr int kCubeCarried = 0, kCubeFixed = 1;  // IKG_CUBE_* (include/ikgrasp.h)
// a minimum over no pairs (ikg_distance_kernel's starting value): clearance not computed
constexpr double kNoClearance = 1e30;

// t_k = t_min + k (t_max - t_min) / (S - 1), t_{S-1} = t_max exactly.  No
// contraction: the host and the device form the same time.
IKG_HD inline double trajcheck_time(double t_min, double t_max, int S, int k) {
#pragma clang fp contract(off)
  return k == S - 1 ? t_max : t_min + ((double)k * (t_max - t_min)) / (double)(S - 1);
}

// World placement of effector h (oMf = oMi[last arm joint] * hand placement)
// from the world joint frames F (joint_world).
template <typename T>
IKG_HD inline void effector_world(const KModel<T>* __restrict__ m, int h, const T (*F)[12], T* E) {
  const T* Fj = F[m->arm_q[h][kArmDof - 1]];
  T d[3];
  matmul3(Fj, m->hand_R[h], E);
  matvec3(Fj, m->hand_t[h], d);
  for (int i = 0; i < 3; ++i) E[9 + i] = Fj[9 + i] + d[i];
}

// The carried cube: oMcube = oM(left effector) * hook_L^-1, the inverse of
// hook_target for arm 0 (the left hand's IK error is zero there).
template <typename T>
IKG_HD inline void carried_cube(const KModel<T>* __restrict__ m, const T* E, T* cube) {
  T d[3];
  matmul3_nt(E, m->hook_R[0], cube);
  matvec3(cube, m->hook_t[0], d);
  for (int i = 0; i < 3; ++i) cube[9 + i] = E[9 + i] - d[i];
}

// norm(log6(oMhand^-1 * oMcube * hook)) of hand h (inverse_geometry.py:66-67):
// what the IK compares with EPSILON.
template <typename T>
IKG_HD inline T grasp_norm(const KModel<T>* __restrict__ m, int h, const T* E, const T* cube) {
  T RT[9], tT[3], Rm[9], d[3], p[3], e[6];
  hook_target(m, h, cube, RT, tT);
  matmul3_tn(E, RT, Rm);
  for (int i = 0; i < 3; ++i) d[i] = tT[i] - E[9 + i];
  matvec3_t(E, d, p);
  // theta / sin(theta) as Pinocchio forms it (kRefRatio, ikg_device.hpp): a drifting grasp sits in
  // the band of small rotation angles where the default's theta / (|skew| / 2) keeps acos's error
  log6<T, true>(Rm, p, e);
  T s = T(0);
  for (int i = 0; i < 6; ++i) s += e[i] * e[i];
  return sqrt(s);
}

// joint j's share of tools.jointlimitscost (tools.py:12-15)
template <typename T>
IKG_HD inline T limit_excess(const KModel<T>* __restrict__ m, int j, T q) {
  return fmax(T(0), fmax(q - m->hi[j], m->lo[j] - q));
}

// A run of consecutive samples of one curve, folded: what a wave leaves in the
// scratch and what the per-curve outputs are made of.
struct TrajPartial {
  int32_t first_collision, first_pair, n_collision;
  int32_t arg_clearance, arg_grasp, arg_limit;
  double min_clearance, max_grasp, max_limit;
};

IKG_HD inline void partial_init(TrajPartial& p) {
  p.first_collision = p.first_pair = -1;
  p.n_collision = 0;
  p.arg_clearance = p.arg_grasp = p.arg_limit = -1;
  p.min_clearance = kNoClearance;
  p.max_grasp = p.max_limit = -1.0;
}

// `b` holds samples after those of `a`: the lowest sample keeps an exact tie
IKG_HD inline void partial_merge(TrajPartial& a, const TrajPartial& b) {
  if (a.first_collision < 0) {
    a.first_collision = b.first_collision;
    a.first_pair = b.first_pair;
  }
  a.n_collision += b.n_collision;
  if (b.arg_clearance >= 0 && (a.arg_clearance < 0 || b.min_clearance < a.min_clearance)) {
    a.min_clearance = b.min_clearance;
    a.arg_clearance = b.arg_clearance;
  }
  if (b.arg_grasp >= 0 && (a.arg_grasp < 0 || b.max_grasp > a.max_grasp)) {
    a.max_grasp = b.max_grasp;
    a.arg_grasp = b.arg_grasp;
  }
  if (b.arg_limit >= 0 && (a.arg_limit < 0 || b.max_limit > a.max_limit)) {
    a.max_limit = b.max_limit;
    a.arg_limit = b.arg_limit;
  }
}

// sample k (after every sample folded so far); pair = the check's witness where it collided
IKG_HD inline void partial_add(TrajPartial& a, int k, bool collides, int pair, bool has_clearance, double clearance,
                               double grasp, double limit) {
  TrajPartial b;
  partial_init(b);
  if (collides) {
    b.first_collision = k;
    b.first_pair = pair;
    b.n_collision = 1;
  }
  if (has_clearance) {
    b.min_clearance = clearance;
    b.arg_clearance = k;
  }
  b.max_grasp = grasp;
  b.arg_grasp = k;
  b.max_limit = limit;
  b.arg_limit = k;
  partial_merge(a, b);
}

// Samples per wave where the caller leaves it open: the shortest run that still
// gives about kTrajWaves waves, so that a small batch fills the device: the
// kernel's registers allow one wave per SIMD, 1,024 resident waves on 256 CUs,
// and two rounds of them even out the samples that run a full sweep.  A batch
// of kTrajWaves curves or more gets one wave per curve, the longest run the
// witness can be carried over.
constexpr int64_t kTrajWaves = 2048;
IKG_HD inline int trajcheck_samples_per_wave(int64_t B, int S, int forced) {
  if (forced >= 1) return forced < S ? forced : S;
  const int64_t want = (kTrajWaves + B - 1) / B;  // chunks per curve
  const int64_t spw = (S + want - 1) / want;
  return (int)(spw < 1 ? 1 : (spw > S ? S : spw));
}

struct TrajCheckArgs {
  const double* points;  // [B, n_points, nq]
  const double* bc;      // [n_points] bezier_coeffs
  int n_points;
  double t_min, t_max, mult;
  int S, spw, chunks, cube_mode;
  const double* cube_fixed;  // [B,12] or null
  const int32_t* pair_idx;   // device; n_idx = 0: no clearance
  int n_idx;
  uint8_t* collision;  // per sample, optional
  double *clearance, *grasp, *limit, *cube;
  TrajPartial* part;  // [B * chunks]
};

struct TrajFoldOut {
  int32_t *first_collision, *first_pair, *n_collision;
  double* min_clearance;
  int32_t* arg_clearance;
  double* max_grasp;
  int32_t* arg_grasp;
  double* max_limit;
  int32_t* arg_limit;
};

IKG_HD inline void fold_store(const TrajFoldOut& o, int64_t b, const TrajPartial& p) {
  if (o.first_collision) o.first_collision[b] = p.first_collision;
  if (o.first_pair) o.first_pair[b] = p.first_pair;
  if (o.n_collision) o.n_collision[b] = p.n_collision;
  if (o.min_clearance) o.min_clearance[b] = p.min_clearance;
  if (o.arg_clearance) o.arg_clearance[b] = p.arg_clearance;
  if (o.max_grasp) o.max_grasp[b] = p.max_grasp;
  if (o.arg_grasp) o.arg_grasp[b] = p.arg_grasp;
  if (o.max_limit) o.max_limit[b] = p.max_limit;
  if (o.arg_limit) o.arg_limit[b] = p.arg_limit;
}

hipError_t launch_trajcheck(const KModel<double>* dm, const KCollision<double>* dc, const TrajCheckArgs& a, int64_t B,
                            const TrajFoldOut& o, hipStream_t s);

}  // namespace ikg
