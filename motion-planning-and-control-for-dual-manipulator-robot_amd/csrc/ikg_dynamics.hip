// Controller dynamics (control.py:284-286) for a batch of states in one launch:
//
//   pin.computeAllTerms(model, data, q, vq); M = data.M   -> M   [B,nq,nq]  (:284-285)
//   pin.nonLinearEffects(model, data, q, vq)              -> nle [B,nq]     (:286)
//   nle at zero velocity                                  -> g   [B,nq]
//
// for any joint tree of the model (KModel jR / jt / jaxis / jparent) with the
// body inertias of KInertia; the per-body arithmetic is ikg_dynamics.hpp.
//
// Layout: one lane per (state, body).  A state occupies a group of G lanes
// (G = 16 for nq <= 16, else 32; 64 / G states per 64-lane workgroup) and each
// lane keeps its own body's placement, velocity, acceleration, world inertia
// and force in registers: nothing is indexed at run time, so nothing spills.
// Lanes exchange bodies with ds_bpermute (__shfl):
//   * forward pass: `levels` rounds in which every lane rebuilds its body from
//     its parent's current state; after round d every body of depth <= d is
//     final (the values of finished bodies are recomputed identically);
//   * in the world frame inertias and forces of a subtree add without
//     transport, so lane i sums the bodies j of its subtree over j = 0..nq-1
//     (ancestor bit masks from the table, scalar loads);
//   * M_ij = S_j . (Ic_i S_i) for j = i or an ancestor of i, written with its
//     mirror entry into the workgroup's dense LDS tile (zeroed first), which
//     is streamed out with 16-byte stores (ikg_control.hip tile_store).
#include <hip/hip_runtime.h>

#include "ikg_dynamics.hpp"
#include "ikg_launch.hpp"

namespace ikg {

namespace {

template <typename T>
__device__ inline T lane_get(T x, int src) {
  return __shfl(x, src, 64);
}

template <typename T, int N>
__device__ inline void lane_get_n(const T (&x)[N], int src, T (&y)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) y[i] = lane_get(x[i], src);
}

// 16-byte coalesced copy of a finished LDS tile to global memory
template <typename T>
__device__ inline void tile_store(const T* __restrict__ tile, T* __restrict__ dst, int n) {
  const int lane = threadIdx.x;
  if ((((uintptr_t)dst) & 15) == 0 && ((n * (int)sizeof(T)) & 15) == 0) {
    const int nv = n * (int)sizeof(T) / 16;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* s = reinterpret_cast<const u32x4*>(tile);
    u32x4* d = reinterpret_cast<u32x4*>(dst);
    for (int i = lane; i < nv; i += 64) __builtin_nontemporal_store(s[i], d + i);
  } else {
    for (int i = lane; i < n; i += 64) dst[i] = tile[i];
  }
}

}  // namespace

template <typename T, int G>
__global__ __launch_bounds__(64) void ikg_dynamics_kernel(const KModel<T>* __restrict__ m,
                                                          const KInertia<T>* __restrict__ in,
                                                          const T* __restrict__ q, const T* __restrict__ v,
                                                          int64_t B, DynOut o) {
  extern __shared__ __align__(16) unsigned char smem[];
  T* tile = reinterpret_cast<T*>(smem);
  constexpr int kStates = 64 / G;
  const int nq = m->nq;
  const int lane = threadIdx.x;
  const int grp = lane / G, b = lane % G, gbase = grp * G;
  const int64_t p0 = (int64_t)blockIdx.x * kStates;
  const int ns = (int)min((int64_t)kStates, B - p0);
  const int64_t p = p0 + grp;
  const bool body = b < nq;
  const bool live = body && grp < ns;
  const int per_state = nq * nq;
  if (o.M) {
    for (int i = lane; i < kStates * per_state; i += 64) tile[i] = T(0);
  }
  // this lane's joint and body (idle lanes: a massless joint under the universe)
  const int bi = body ? b : 0;
  T jR[9], jt[3], h[3], Io[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) jR[i] = m->jR[bi][i];
#pragma unroll
  for (int i = 0; i < 3; ++i) jt[i] = m->jt[bi][i];
#pragma unroll
  for (int i = 0; i < 3; ++i) h[i] = body ? in->h[bi][i] : T(0);
#pragma unroll
  for (int i = 0; i < 6; ++i) Io[i] = body ? in->Io[bi][i] : T(0);
  const T mass = body ? in->mass[bi] : T(0);
  const int axis = m->jaxis[bi];
  const int parent = body ? m->jparent[bi] : -1;
  const uint32_t anc = body ? in->anc[bi] : 0u;
  const T grav[3] = {in->grav[0], in->grav[1], in->grav[2]};
  const T ref[3] = {in->ref[0], in->ref[1], in->ref[2]};
  const int levels = in->levels;
  T s, c;
  cw_sincos(live ? q[p * nq + b] : T(0), &s, &c);
  const T qd = (live && v) ? v[p * nq + b] : T(0);

  DynBody<T> uni, me;
  dyn_universe(grav, ref, uni);
  me = uni;
  T S[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  const int src = parent >= 0 ? gbase + parent : lane;
#pragma unroll 1
  for (int l = 0; l < levels; ++l) {
    DynBody<T> par;
    lane_get_n(me.R, src, par.R);
    lane_get_n(me.o, src, par.o);
    lane_get_n(me.v, src, par.v);
    lane_get_n(me.a, src, par.a);
    if (parent < 0) par = uni;
    dyn_forward(par, jR, jt, axis, s, c, qd, me, S);
  }
  DynInertia<T> W;
  dyn_inertia_world(mass, h, Io, me.R, me.o, W);
  T f[6], f0[6];
  const T zero[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  dyn_force(W, me.v, me.a, f);
  dyn_force(W, zero, uni.a, f0);

  // subtree sums (j ascending, as dynamics_state)
  DynInertia<T> Ic;
  dyn_inertia_zero(Ic);
  T fc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, gc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  const bool want_f = o.nle != nullptr, want_g = o.g != nullptr, want_M = o.M != nullptr;
#pragma unroll 1
  for (int j = 0; j < nq; ++j) {
    const bool mine = (in->anc[j] >> b) & 1;  // j in the subtree of b
    if (want_M) {
      DynInertia<T> Wj;
      Wj.m = lane_get(W.m, gbase + j);
      lane_get_n(W.h, gbase + j, Wj.h);
      lane_get_n(W.I, gbase + j, Wj.I);
      if (mine) dyn_inertia_add(Ic, Wj);
    }
    if (want_f) {
      T fj[6];
      lane_get_n(f, gbase + j, fj);
      if (mine) {
#pragma unroll
        for (int k = 0; k < 6; ++k) fc[k] += fj[k];
      }
    }
    if (want_g) {
      T gj[6];
      lane_get_n(f0, gbase + j, gj);
      if (mine) {
#pragma unroll
        for (int k = 0; k < 6; ++k) gc[k] += gj[k];
      }
    }
  }
  if (live && want_f) ((T*)o.nle)[p * nq + b] = ddot6(S, fc);
  if (live && want_g) ((T*)o.g)[p * nq + b] = ddot6(S, gc);
  if (want_M) {
    T F[6];
    dyn_apply(Ic, S, F);
    __syncthreads();  // the tile is zeroed
    T* Mt = tile + grp * per_state;
#pragma unroll 1
    for (int j = 0; j < nq; ++j) {
      T Sj[6];
      lane_get_n(S, gbase + j, Sj);
      if (live && ((anc >> j) & 1)) {
        const T x = ddot6(Sj, F);
        Mt[b * nq + j] = x;
        Mt[j * nq + b] = x;
      }
    }
    __syncthreads();
    tile_store(tile, (T*)o.M + p0 * per_state, ns * per_state);
  }
}

template <typename T, int G>
static hipError_t launch_dynamics_g(const KModel<T>* dm, const KInertia<T>* di, int nq, const T* q, const T* v,
                                    int64_t B, const DynOut& o, hipStream_t s) {
  constexpr int kStates = 64 / G;
  const int64_t nblocks = (B + kStates - 1) / kStates;
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  const size_t lds = o.M ? sizeof(T) * kStates * nq * nq : 0;
  hipLaunchKernelGGL((ikg_dynamics_kernel<T, G>), dim3((unsigned)nblocks), dim3(64), lds, s, dm, di, q, v, B, o);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_dynamics(const KModel<T>* dm, const KInertia<T>* di, int nq, const void* q, const void* v,
                           int64_t B, const DynOut& o, hipStream_t s) {
  if (B <= 0 || !(o.M || o.nle || o.g)) return hipSuccess;
  if (nq <= 16) return launch_dynamics_g<T, 16>(dm, di, nq, (const T*)q, (const T*)v, B, o, s);
  return launch_dynamics_g<T, 32>(dm, di, nq, (const T*)q, (const T*)v, B, o, s);
}

// ---------------------------------------------------------------- controller solve
// One lane per (state, row): a state's matrices live in its slice of LDS
// (CtlWs, 7.3 KB at nq = 15) and its G lanes run the phases of
// ikg_dynamics.hpp with a barrier between phases (a workgroup is one wave).
// Groups past the end of the batch work on the last state and store nothing.
template <int G>
__global__ __launch_bounds__(64) void ikg_control_solve_kernel(CtlIn in, int nq, int64_t B, KCtl<double> prm,
                                                               CtlOut o) {
  using T = double;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int grp = lane / G, r = lane % G;
  const int64_t p0 = (int64_t)blockIdx.x * (64 / G);
  const bool live = p0 + grp < B;
  const int64_t p = live ? p0 + grp : B - 1;
  CtlWs<T> w;
  ctl_ws_bind(reinterpret_cast<T*>(smem) + (size_t)grp * ctl_ws_len(nq), nq, w);
  const T* gM = (const T*)in.M + p * nq * nq;
  const T* gJ = (const T*)in.J + p * 12 * nq;
  for (int i = r; i < nq * nq; i += G) w.M[(i / nq) * w.ld + i % nq] = gM[i];
  for (int i = r; i < 12 * nq; i += G) w.J[(i / nq) * w.ld + i % nq] = gJ[i];
  if (r < nq) {
    w.Md[r] = gM[r * nq + r];
    w.nle[r] = ((const T*)in.nle)[p * nq + r];
  }
  if (r < 12) {
    w.dJv[r] = ((const T*)in.dJv)[p * 12 + r];
    w.e[r] = ((const T*)in.err)[p * 12 + r];
    w.ed[r] = ((const T*)in.derr)[p * 12 + r];
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < nq; ++k) {
    ldl_step(w.M, w.ld, nq, k, r);
    __syncthreads();
  }
  ctl_pivots(w, r);
  __syncthreads();
  ctl_forward(w, prm, r);
  __syncthreads();
  ctl_opspace(w, prm, r);
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < 6; ++k) {
    ctl_opspace_step(w, k, r);
    __syncthreads();
  }
  T lam[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  ctl_lambda(w, prm, r, lam);
  __syncthreads();
  ctl_normal(w, prm, r);
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < nq; ++k) {
    ldl_step(w.H, w.ld, nq, k, r);
    __syncthreads();
  }
  ctl_check(w, r);
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < nq; ++k) {
    ctl_solve_fwd(w, k, r);
    __syncthreads();
  }
#pragma unroll 1
  for (int k = nq - 1; k >= 0; --k) {
    ctl_solve_bwd(w, k, r);
    __syncthreads();
  }
  if (!live) return;
  if (r < nq) {
    const T t = ctl_tau(w, prm, r);
    if (o.tau) ((T*)o.tau)[p * nq + r] = t;
    if (o.qdd) ((T*)o.qdd)[p * nq + r] = w.qdd[r];
  }
  if (r < 12) {
    if (o.xdd) ((T*)o.xdd)[p * 12 + r] = w.xdd[r];
    if (o.fc) ((T*)o.fc)[p * 12 + r] = w.fc[r];
    if (o.Lambda) {
#pragma unroll
      for (int b = 0; b < 6; ++b) ((T*)o.Lambda)[p * 72 + r * 6 + b] = lam[b];
    }
  }
}

hipError_t launch_control_solve(const CtlIn& in, int nq, int64_t B, const KCtl<double>& prm, const CtlOut& o,
                                hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const int G = nq <= 16 ? 16 : 32;
  const int64_t nblocks = (B + 64 / G - 1) / (64 / G);
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  const size_t lds = sizeof(double) * (64 / G) * ctl_ws_len(nq);
  if (G == 16)
    hipLaunchKernelGGL((ikg_control_solve_kernel<16>), dim3((unsigned)nblocks), dim3(64), lds, s, in, nq, B, prm, o);
  else
    hipLaunchKernelGGL((ikg_control_solve_kernel<32>), dim3((unsigned)nblocks), dim3(64), lds, s, in, nq, B, prm, o);
  return hipGetLastError();
}

template hipError_t launch_dynamics<double>(const KModel<double>*, const KInertia<double>*, int, const void*,
                                            const void*, int64_t, const DynOut&, hipStream_t);
template hipError_t launch_dynamics<float>(const KModel<float>*, const KInertia<float>*, int, const void*,
                                           const void*, int64_t, const DynOut&, hipStream_t);

}  // namespace ikg
