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

hipError_t launch_se3_interpolate(const double* A, const double* B, const double* alpha, int64_t C, double* out,
                                  hipStream_t s);
hipError_t launch_nearest(const double* nodes, int64_t cap, const int32_t* counts, const double* queries, int nq,
                          int64_t P, int32_t* index, double* dist, hipStream_t s);
hipError_t launch_project_prepare(const KCollision<double>* dc, const ProjectArgs& a, int step, hipStream_t s);
hipError_t launch_project_commit(const ProjectArgs& a, int step, hipStream_t s);

}  // namespace ikg
