// Batched Bezier trajectory fit, the reference's maketraj (control.py:63-197)
// solved exactly: one 256-lane workgroup per path, the augmented matrix
// [A_f | rhs; sqrt(ridge) 1 | 0] of ikg_fit.hpp in LDS (up to 271 x 47 doubles:
// dynamic LDS above the 64 KiB default, inside the CU's 160 KiB), a Householder
// reflection per free control point with the right-hand sides of all joints
// carried along, a back substitution per joint, then the derivative control
// points and the cost with the reference's Horner.  A path is independent of
// its neighbours and its sums run in a fixed order: its result does not depend
// on the batch it is solved in.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ikg_fit.hpp"
#include "ikg_launch.hpp"

namespace ikg {

namespace {

// the phase executor of ikg_fit.hpp in a kernel: items strided over the workgroup, a barrier ends the phase
struct LaneItems {
  template <typename F>
  __device__ void operator()(int count, F&& fn) {
    for (int i = threadIdx.x; i < count; i += kFitLanes) fn(i);
    __syncthreads();
  }
};

}  // namespace

__global__ __launch_bounds__(kFitLanes) void ikg_bezier_fit_kernel(FitArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int64_t p = blockIdx.x;
  const int64_t first = a.offsets[p];
  const int64_t n = a.offsets[p + 1] - first;
  // the count is checked before it sizes or indexes anything (uniform over the workgroup)
  if (!fit_count_ok(n, a.degree, a.ridge)) {
    if (threadIdx.x == 0) {
      a.status[p] = 1;
      fit_store_nan(a.cost + p);
    }
    return;
  }
  const int d = a.degree, dim = a.dim;
  FitWs w;
  fit_ws_bind(reinterpret_cast<double*>(smem), d, dim, w);
  const FitPath f{a.q0 + p * dim, a.q1 + p * dim, a.y + first * dim, (int)n, dim, d, a.ridge, a.T, a.bc};
  LaneItems ex;
  const double cost = bezier_fit_path(f, w, ex, a.points + p * (d + 1) * dim,
                                      a.vpoints ? a.vpoints + p * d * dim : nullptr,
                                      a.apoints ? a.apoints + p * (d - 1) * dim : nullptr);
  if (threadIdx.x == 0) {
    a.status[p] = 0;
    a.cost[p] = cost;
  }
}

hipError_t launch_bezier_fit(const FitArgs& args, int64_t B, hipStream_t s) {
  const size_t lds = sizeof(double) * fit_ws_len(args.degree, args.dim);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute((const void*)ikg_bezier_fit_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int64_t chunk = (int64_t)1 << 20;  // paths per launch
  for (int64_t off = 0; off < B; off += chunk) {
    FitArgs a = args;
    a.q0 += off * a.dim;
    a.q1 += off * a.dim;
    a.offsets += off;
    a.points += off * (a.degree + 1) * a.dim;
    if (a.vpoints) a.vpoints += off * a.degree * a.dim;
    if (a.apoints) a.apoints += off * (a.degree - 1) * a.dim;
    a.cost += off;
    a.status += off;
    hipLaunchKernelGGL(ikg_bezier_fit_kernel, dim3((unsigned)std::min(chunk, B - off)), dim3(kFitLanes), lds, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ikg
