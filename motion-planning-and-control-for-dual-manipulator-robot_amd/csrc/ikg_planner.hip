// Kernels of the RRT-Connect planner (ikg_planner.hpp): SE3.Interpolate over a
// batch, nearest tree node per planner, and the prepare / commit steps that
// bracket the IK solve of the device-side path projection (ikg_capi.hip
// ikg_project_paths).  fp64 only: the planner's IK is fp64.
#include <hip/hip_runtime.h>

#include "ikg_planner.hpp"

namespace ikg {

__global__ __launch_bounds__(256) void ikg_se3_interpolate_kernel(const double* __restrict__ A,
                                                                  const double* __restrict__ B,
                                                                  const double* __restrict__ alpha, int64_t C,
                                                                  double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C) return;
  double a[12], b[12], o[12];
  for (int k = 0; k < 12; ++k) {
    a[k] = A[12 * i + k];
    b[k] = B[12 * i + k];
  }
  se3_interpolate(a, b, alpha[i], o);
  for (int k = 0; k < 12; ++k) out[12 * i + k] = o[k];
}

// One 64-lane wave per tree: lanes stride over the rows (ascending, so a lane
// keeps the lowest index of its own ties), then a shuffle argmin over (d2, index).
__global__ __launch_bounds__(64) void ikg_nearest_kernel(const double* __restrict__ nodes, int64_t cap,
                                                         const int32_t* __restrict__ counts,
                                                         const double* __restrict__ queries, int nq, int64_t P,
                                                         int32_t* __restrict__ index, double* __restrict__ dist) {
  const int64_t p = blockIdx.x;
  if (p >= P) return;
  const int lane = threadIdx.x;
  const int64_t n = counts[p] < cap ? counts[p] : cap;  // never past the tree's storage
  const double* tree = nodes + p * cap * nq;
  const double* qy = queries + p * nq;
  double d2 = DBL_MAX;
  int best = -1;
  for (int64_t r = lane; r < n; r += 64) {
    const double d = row_dist2(tree + r * nq, qy, nq);
    if (nearest_takes(d2, best, d, (int)r)) {
      d2 = d;
      best = (int)r;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(d2, off);
    const int ob = __shfl_xor(best, off);
    if (nearest_takes(d2, best, od, ob)) {
      d2 = od;
      best = ob;
    }
  }
  if (lane == 0) {
    index[p] = best;
    dist[p] = best >= 0 ? sqrt(d2) : 0.0;
  }
}

// Step `step` (1-based) of every chain, before the solve: one thread per chain.
__global__ __launch_bounds__(256) void ikg_project_prepare_kernel(const KCollision<double>* __restrict__ c,
                                                                  const ProjectArgs a, int step) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.C) return;
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

// After the solve: append where the chain was live, its placement free and the
// solve converged; otherwise stop the chain.
__global__ __launch_bounds__(256) void ikg_project_commit_kernel(const ProjectArgs a, int step) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.C) return;
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

hipError_t launch_se3_interpolate(const double* A, const double* B, const double* alpha, int64_t C, double* out,
                                  hipStream_t s) {
  if (C <= 0) return hipSuccess;
  hipLaunchKernelGGL(ikg_se3_interpolate_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, A, B, alpha, C,
                     out);
  return hipGetLastError();
}

hipError_t launch_nearest(const double* nodes, int64_t cap, const int32_t* counts, const double* queries, int nq,
                          int64_t P, int32_t* index, double* dist, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  hipLaunchKernelGGL(ikg_nearest_kernel, dim3((unsigned)P), dim3(64), 0, s, nodes, cap, counts, queries, nq, P, index,
                     dist);
  return hipGetLastError();
}

hipError_t launch_project_prepare(const KCollision<double>* dc, const ProjectArgs& a, int step, hipStream_t s) {
  if (a.C <= 0) return hipSuccess;
  hipLaunchKernelGGL(ikg_project_prepare_kernel, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, s, dc, a, step);
  return hipGetLastError();
}

hipError_t launch_project_commit(const ProjectArgs& a, int step, hipStream_t s) {
  if (a.C <= 0) return hipSuccess;
  hipLaunchKernelGGL(ikg_project_commit_kernel, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, s, a, step);
  return hipGetLastError();
}

}  // namespace ikg
