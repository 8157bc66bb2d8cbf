// RRT-Connect planner primitives (path.py:125-278): SE3.Interpolate, the
// nearest-neighbour rule of the planner's trees and the step bookkeeping of
// the device-side path projection.  The device functions are IKG_HD so the
// host emulator (ikg_host_emu.hip) runs the same arithmetic on the CPU.
#pragma once

#include <float.h>

#include "ikg_collision.hpp"
#include "ikg_device.hpp"
#include "ikg_ws_layout.hpp"

namespace ikg {

// pin.exp6 of [v; w] (Pinocchio spatial/explog.hpp): the Taylor branch below
// precision<3>() = eps^(1/4), as ikgrasp/se3.py and oracle/planner_oracle.py.
template <typename T>
IKG_HD inline void exp6(const T* e, T* R, T* p) {
  const T* w = e + 3;
  const T t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const T t = sqrt(t2);
  T a, b, c;
  if (t < T(Prec<T>::kPrec3)) {
    a = T(1) - t2 / T(6);
    b = T(0.5) - t2 / T(24);
    c = T(1) / T(6) - t2 / T(120);
  } else {
    T st, ct;
    Prec<T>::sincos_(t, &st, &ct);
    a = st / t;
    b = (T(1) - ct) / t2;
    c = (t - st) / (t2 * t);
  }
  // W = skew(w), W2 = W W = w w^T - |w|^2 1
  const T W[9] = {T(0), -w[2], w[1], w[2], T(0), -w[0], -w[1], w[0], T(0)};
  T W2[9];
  matmul3(W, W, W2);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? T(1) : T(0)) + a * W[i] + b * W2[i];
  T V[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0 ? T(1) : T(0)) + b * W[i] + c * W2[i];
  matvec3(V, e, p);
}

// pin.SE3.Interpolate(A, B, alpha) = A * exp6(alpha * log6(A^-1 B)) on
// placements [12] = R row-major, then t (path.py:141)
template <typename T>
IKG_HD inline void se3_interpolate(const T* A, const T* B, T alpha, T* out) {
  T Rm[9], d[3], pm[3], e[6], Re[9], pe[3], u[3];
  matmul3_tn(A, B, Rm);
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = B[9 + i] - A[9 + i];
  matvec3_t(A, d, pm);
  log6<T, true>(Rm, pm, e);  // theta/sin(theta) as Pinocchio forms it (ikg_device.hpp)
#pragma unroll
  for (int i = 0; i < 6; ++i) e[i] *= alpha;
  exp6(e, Re, pe);
  matmul3(A, Re, out);
  matvec3(A, pe, u);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[9 + i] = A[9 + i] + u[i];
}

// squared Euclidean distance of one tree row to the query, j = 0 .. nq-1 in order
IKG_HD inline double row_dist2(const double* row, const double* query, int nq) {
  double d2 = 0.0;
  for (int j = 0; j < nq; ++j) {
    const double d = row[j] - query[j];
    d2 += d * d;
  }
  return d2;
}

// The argmin over (d2, index): the lesser distance, the lower index among
// exact ties; index < 0 = no candidate.  Whether (d2b, ib) replaces (d2a, ia).
IKG_HD inline bool nearest_takes(double d2a, int ia, double d2b, int ib) {
  return ib >= 0 && (ia < 0 || d2b < d2a || (d2b == d2a && ib < ia));
}

// path.py:129-130: int(|dt| / step_size) + 1
IKG_HD inline int projection_steps(const double* a, const double* b, double step_size) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (int)(sqrt(dx * dx + dy * dy + dz * dz) / step_size) + 1;
}

// ikg_project_paths: status of a chain (include/ikgrasp.h); kLive while it is advancing
constexpr int kPathReached = 0, kPathCollision = 1, kPathIkFailed = 2, kPathCut = 3, kPathLive = -1;

// the world-fixed geometries of the placement check, by value to the kernel
struct GeomList {
  int32_t n;
  int32_t g[kMaxGeoms];
};

// scratch of one ikg_project_paths call: the step's targets, warm starts and
// solve outputs, and per chain its step count and whether the step's placement is free
struct ProjectLayout : WsLayout {
  int targets, q0, q, err, iters, conv, aux;
  ProjectLayout(size_t C, size_t nq)
      : targets(add(8 * 12 * C, kFloat)), q0(add(8 * nq * C, kFloat)), q(add(8 * nq * C, kFloat)),
        err(add(8 * 2 * C, kFloat)), iters(add(4 * C, kInt)), conv(add(C, kInt)), aux(add(4 * 2 * C, kInt)) {}
};

struct ProjectArgs {
  const double *q_curr, *cube_curr, *cube_rand;  // [C,nq], [C,12], [C,12]
  int64_t C;
  int nq, max_nodes;
  double step_size;
  GeomList geoms;
  double *robot_path, *cube_path;  // [C,max_nodes,nq], [C,max_nodes,12]
  int32_t *n_nodes, *status;       // [C]
  // scratch (ProjectLayout)
  double *targets, *q0;
  const double* q;
  const uint8_t* conv;
  int32_t *steps, *free_;
};

// Step `step` (1-based) of chain i, before the solve: row 0 and the step count
// at step 1, then the step's target (where the chain is live and its placement
// free) or the chain's last accepted row, and the warm start.
IKG_HD inline void project_prepare_chain(const KCollision<double>* __restrict__ c, const ProjectArgs& a, int64_t i, int step) {
  const int nq = a.nq;
  double* rp = a.robot_path + i * a.max_nodes * nq;
  double* cp = a.cube_path + i * a.max_nodes * 12;
  const double* A = a.cube_curr + 12 * i;
  const double* B = a.cube_rand + 12 * i;
  if (step == 1) {  // row 0 and the chain's step count
    for (int k = 0; k < nq; ++k) rp[k] = a.q_curr[i * nq + k];
    for (int k = 0; k < 12; ++k) cp[k] = A[k];
    a.steps[i] = projection_steps(A + 9, B + 9, a.step_size);
    a.n_nodes[i] = 1;
    a.status[i] = a.max_nodes > 1 ? kPathLive : kPathCut;
  }
  int n = a.n_nodes[i];  // 1 <= n <= max_nodes by construction; the reads below are bounded regardless
  n = n < 1 ? 1 : (n > a.max_nodes ? a.max_nodes : n);
  const double* last_q = rp + (int64_t)(n - 1) * nq;
  const double* last_p = cp + (int64_t)(n - 1) * 12;
  double* tg = a.targets + 12 * i;
  int free_ = 0;
  if (a.status[i] == kPathLive) {  // then step <= steps: the commit ends a chain at step == steps
    double P[12];
    se3_interpolate(A, B, (double)step / (double)a.steps[i], P);
    const int tgm = c->target_geom;
    const Shape<double> S{P, P + 9, c->dims[tgm], c->kind[tgm]};
    int hit = 0;
    for (int k = 0; k < a.geoms.n; ++k) {
      const int g = a.geoms.g[k];
      const Shape<double> E{c->R[g], c->t[g], c->dims[g], c->kind[g]};
      hit |= pair_collides(S, E) != 0;
    }
    free_ = !hit;
    if (free_)
      for (int k = 0; k < 12; ++k) tg[k] = P[k];
  }
  // a chain that is stopped, finished or in collision here: its last accepted
  // placement and q, which the solve leaves after 0 updates
  if (!free_)
    for (int k = 0; k < 12; ++k) tg[k] = last_p[k];
  for (int k = 0; k < nq; ++k) a.q0[i * nq + k] = last_q[k];
  a.free_[i] = free_;
}

// Chain i after the solve: append where the chain was live, its placement free
// and the solve converged; otherwise stop the chain.
IKG_HD inline void project_commit_chain(const ProjectArgs& a, int64_t i, int step) {
  if (a.status[i] != kPathLive) return;
  if (!a.free_[i]) {
    a.status[i] = kPathCollision;
    return;
  }
  if (!a.conv[i]) {
    a.status[i] = kPathIkFailed;
    return;
  }
  const int n = a.n_nodes[i];
  if (n < 1 || n >= a.max_nodes) {  // the write index is bounded before the store
    a.status[i] = kPathCut;
    return;
  }
  const int nq = a.nq;
  double* rq = a.robot_path + (i * a.max_nodes + n) * nq;
  double* rc = a.cube_path + (i * a.max_nodes + n) * 12;
  for (int k = 0; k < nq; ++k) rq[k] = a.q[i * nq + k];
  for (int k = 0; k < 12; ++k) rc[k] = a.targets[12 * i + k];
  a.n_nodes[i] = n + 1;
  if (step >= a.steps[i])
    a.status[i] = kPathReached;
  else if (n + 1 >= a.max_nodes)
    a.status[i] = kPathCut;
}

// Steps a host-pointer ikg_project_paths enqueues: every chain ends within
// max_nodes - 1 steps, and the host knows the longest chain (one spare step
// against a last-bit difference of the device's own count; a finished chain's
// extra step changes nothing).  -1 with *bad = the chain whose |dt| / step_size
// is too large for a count.
inline int64_t projection_host_steps(const double* cube_curr, const double* cube_rand, int64_t C, double step_size,
                                     int32_t max_nodes, int64_t* bad) {
  int64_t longest = 0;
  for (int64_t c = 0; c < C; ++c) {
    const double *pa = cube_curr + 12 * c + 9, *pb = cube_rand + 12 * c + 9;
    if (!(sqrt((pa[0] - pb[0]) * (pa[0] - pb[0]) + (pa[1] - pb[1]) * (pa[1] - pb[1]) +
               (pa[2] - pb[2]) * (pa[2] - pb[2])) / step_size < 1e9)) {
      *bad = c;
      return -1;
    }
    const int64_t n = (int64_t)projection_steps(pa, pb, step_size * (1.0 - 1e-12));
    longest = n > longest ? n : longest;
  }
  const int64_t cap = (int64_t)max_nodes - 1;
  return cap < longest ? cap : longest;
}

hipError_t launch_se3_interpolate(const double* A, const double* B, const double* alpha, int64_t C, double* out,
                                  hipStream_t s);
hipError_t launch_nearest(const double* nodes, int64_t cap, const int32_t* counts, const double* queries, int nq,
                          int64_t P, int32_t* index, double* dist, hipStream_t s);
hipError_t launch_project_prepare(const KCollision<double>* dc, const ProjectArgs& a, int step, hipStream_t s);
hipError_t launch_project_commit(const ProjectArgs& a, int step, hipStream_t s);

}  // namespace ikg
