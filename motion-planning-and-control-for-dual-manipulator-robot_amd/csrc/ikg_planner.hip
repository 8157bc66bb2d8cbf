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

// Step `step` (1-based) of every chain, before the solve: one thread per chain
// (project_prepare_chain, ikg_planner.hpp).
__global__ __launch_bounds__(256) void ikg_project_prepare_kernel(const KCollision<double>* __restrict__ c,
                                                                  const ProjectArgs a, int step) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.C) return;
  project_prepare_chain(c, a, i, step);
}

// After the solve: one thread per chain (project_commit_chain).
__global__ __launch_bounds__(256) void ikg_project_commit_kernel(const ProjectArgs a, int step) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.C) return;
  project_commit_chain(a, i, step);
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
