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
//
// Further down: the controller solve (control.py:348-406), forward dynamics
// qdd = M^-1 (tau - nle), the Bezier desired state (control.py:30-46) and the
// per-tick step kernel of the closed-loop rollout (control.py:461-463), and
// inverse dynamics with the actuator-limit ratios along Bezier curves
// (ikg_trajectory_dynamics_batch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "ikg_dynamics.hpp"
#include "ikg_launch.hpp"
#include "ikg_trajcheck.hpp"

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

// The phase executor of ikg_dynamics.hpp in a kernel: lane r runs row r, a
// barrier ends the phase (a workgroup is one wave).  The lane's row of Lambda
// stays in its registers.
template <typename T>
struct LaneRows {
  int r;
  T lam_[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  template <typename F>
  __device__ void operator()(F&& fn) {
    fn(r);
    __syncthreads();
  }
  __device__ T* lam(int) { return lam_; }
};

// state p of the scratch -> its workspace, spread over the state's G lanes (no barrier)
template <typename T>
__device__ inline void ctl_ws_load_lanes(const CtlWs<T>& w, const CtlIn& in, int64_t p, int r, int G) {
  const int nq = w.nq;
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
}

// The geometry of every kernel here: G lanes per state (16 for nq <= 16, else
// 32), one wave per workgroup.  launch(g, nblocks) starts the kernel
// specialised for G = g.value and returns its status.
template <typename F>
hipError_t launch_per_state(int nq, int64_t B, F&& launch) {
  if (B <= 0) return hipSuccess;
  const int states = nq <= 16 ? 4 : 2;
  const int64_t nblocks = (B + states - 1) / states;
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  return nq <= 16 ? launch(std::integral_constant<int, 16>{}, (unsigned)nblocks)
                  : launch(std::integral_constant<int, 32>{}, (unsigned)nblocks);
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

  // (the forward pass is written out here and in the forward-dynamics kernel: as
  // one shared function it moved fp64 M, nle, g in the last bit with the joint
  // loads inside, and cost this kernel 1.7 % with only the rounds inside)
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

template <typename T>
hipError_t launch_dynamics(const KModel<T>* dm, const KInertia<T>* di, int nq, const void* q, const void* v,
                           int64_t B, const DynOut& o, hipStream_t s) {
  if (!(o.M || o.nle || o.g)) return hipSuccess;
  return launch_per_state(nq, B, [&](auto g, unsigned nblocks) {
    constexpr int G = decltype(g)::value;
    const size_t lds = o.M ? sizeof(T) * (64 / G) * nq * nq : 0;
    hipLaunchKernelGGL((ikg_dynamics_kernel<T, G>), dim3(nblocks), dim3(64), lds, s, dm, di, (const T*)q,
                       (const T*)v, B, o);
    return hipGetLastError();
  });
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
  ctl_ws_load_lanes(w, in, p, r, G);
  __syncthreads();
  LaneRows<T> rows{r};
  control_solve_phases(w, prm, rows);
  const T(&lam)[6] = rows.lam_;
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
  return launch_per_state(nq, B, [&](auto g, unsigned nblocks) {
    constexpr int G = decltype(g)::value;
    const size_t lds = sizeof(double) * (64 / G) * ctl_ws_len(nq);
    hipLaunchKernelGGL((ikg_control_solve_kernel<G>), dim3(nblocks), dim3(64), lds, s, in, nq, B, prm, o);
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------- forward dynamics
// qdd = M^-1 (tau - nle): the solve kernel's layout (G lanes per state, M in
// LDS, one wave per workgroup), lane b = body b = row b.  nle comes from the
// dynamics kernel (scratch).  M is formed here, each row about its own joint's
// origin (ikg_dynamics.hpp "M about each joint's own origin": the division by M
// needs its small rows to their own relative accuracy), straight into LDS:
// the dynamics kernel's forward pass at zero velocity, then lane b sums the
// bodies of its subtree as seen from o_b and writes row b with its mirror
// entries.  Then the factorisation of M and the two substitutions.
template <int G>
__global__ __launch_bounds__(64) void ikg_forward_dynamics_kernel(const KModel<double>* __restrict__ m,
                                                                  const KInertia<double>* __restrict__ in,
                                                                  const double* __restrict__ q,
                                                                  const double* __restrict__ nle,
                                                                  const double* __restrict__ tau, int64_t B,
                                                                  double* __restrict__ qdd) {
  using T = double;
  extern __shared__ __align__(16) unsigned char smem[];
  const int nq = m->nq;
  const int lane = threadIdx.x;
  const int grp = lane / G, b = lane % G, gbase = grp * G;
  const int64_t p0 = (int64_t)blockIdx.x * (64 / G);
  const bool live = p0 + grp < B;
  const int64_t p = live ? p0 + grp : B - 1;
  const bool body = b < nq;
  CtlWs<T> f;
  fd_ws_bind(reinterpret_cast<T*>(smem) + (size_t)grp * fd_ws_len(nq), nq, f);
  for (int i = b; i < nq * f.ld; i += G) f.M[i] = T(0);
  if (body) f.rhs[b] = tau[p * nq + b] - nle[p * nq + b];
  if (b == 0) *f.fail = T(0);
  // this lane's joint (idle lanes: a joint under the universe that owns no row)
  const int bi = body ? b : 0;
  T jR[9], jt[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) jR[i] = m->jR[bi][i];
#pragma unroll
  for (int i = 0; i < 3; ++i) jt[i] = m->jt[bi][i];
  const int axis = m->jaxis[bi];
  const int parent = body ? m->jparent[bi] : -1;
  const uint32_t anc = body ? in->anc[bi] : 0u;
  const T grav[3] = {in->grav[0], in->grav[1], in->grav[2]};
  const T ref[3] = {in->ref[0], in->ref[1], in->ref[2]};
  const int levels = in->levels;
  T s, c;
  cw_sincos(body ? q[p * nq + b] : T(0), &s, &c);
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
    dyn_forward(par, jR, jt, axis, s, c, T(0), me, S);
  }
  // the subtree of b as seen from o_b (j ascending, as inertia_matrix_local_state)
  DynInertia<T> Ic;
  dyn_inertia_zero(Ic);
#pragma unroll 1
  for (int j = 0; j < nq; ++j) {
    T Rj[9], oj[3];
    lane_get_n(me.R, gbase + j, Rj);
    lane_get_n(me.o, gbase + j, oj);
    const T hj[3] = {in->h[j][0], in->h[j][1], in->h[j][2]};
    const T Ioj[6] = {in->Io[j][0], in->Io[j][1], in->Io[j][2], in->Io[j][3], in->Io[j][4], in->Io[j][5]};
    if (body && ((in->anc[j] >> b) & 1)) dyn_inertia_add_about(in->mass[j], hj, Ioj, Rj, oj, me.o, Ic);
  }
  T Sb[6], F[6];
  dyn_subspace_about(me.o, me.o, S + 3, Sb);
  dyn_apply(Ic, Sb, F);
  __syncthreads();  // M is zeroed
#pragma unroll 1
  for (int j = 0; j < nq; ++j) {
    T oj[3], aj[3];
    lane_get_n(me.o, gbase + j, oj);
    const T a3[3] = {S[3], S[4], S[5]};
    lane_get_n(a3, gbase + j, aj);
    if (body && ((anc >> j) & 1)) {
      T Sj[6];
      dyn_subspace_about(oj, me.o, aj, Sj);
      const T x = ddot6(Sj, F);
      f.M[b * f.ld + j] = x;
      f.M[j * f.ld + b] = x;
    }
  }
  __syncthreads();
  LaneRows<T> rows{b};
  ldl_factor(f.M, f.ld, nq, rows);
  ctl_substitute(f, rows);
  if (live && body) qdd[p * nq + b] = f.qdd[b];
}

hipError_t launch_forward_dynamics(const KModel<double>* dm, const KInertia<double>* di, int nq, const void* q,
                                   const void* nle, const void* tau, int64_t B, void* qdd, hipStream_t s) {
  return launch_per_state(nq, B, [&](auto g, unsigned nblocks) {
    constexpr int G = decltype(g)::value;
    const size_t lds = sizeof(double) * (64 / G) * fd_ws_len(nq);
    hipLaunchKernelGGL((ikg_forward_dynamics_kernel<G>), dim3(nblocks), dim3(64), lds, s, dm, di, (const double*)q,
                       (const double*)nle, (const double*)tau, B, (double*)qdd);
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------- Bezier curves
namespace {

constexpr int kTableChunk = 384;  // doubles per launch: 3 KB of the 4 KB of kernel arguments
struct TableChunk {
  double x[kTableChunk];
};

// state p's curves over the table `tab` (RolloutCurves); PS: a curve pair per state.  A template parameter, not
// a run-time branch: the shared-curve step kernel compiles as it did before the per-state entry existed.
template <bool PS>
__device__ inline KBezier<double> curve_q(const RolloutCurves& cv, const double* tab, int nq, int64_t p) {
  if constexpr (PS)
    return KBezier<double>{cv.pq + p * cv.stride_q, tab, cv.nq_pts, nq, cv.q_tmin, cv.q_tmax, cv.q_mult};
  return KBezier<double>{tab, tab + cv.nq_pts * nq, cv.nq_pts, nq, cv.q_tmin, cv.q_tmax, cv.q_mult};
}
template <bool PS>
__device__ inline KBezier<double> curve_v(const RolloutCurves& cv, const double* tab, int nq, int64_t p) {
  if constexpr (PS)
    return KBezier<double>{cv.pv + p * cv.stride_v, tab + cv.nq_pts, cv.nv_pts, nq, cv.v_tmin, cv.v_tmax, cv.v_mult};
  const double* tv = tab + (size_t)cv.nq_pts * (nq + 1);
  return KBezier<double>{tv, tv + cv.nv_pts * nq, cv.nv_pts, nq, cv.v_tmin, cv.v_tmax, cv.v_mult};
}

}  // namespace

__global__ __launch_bounds__(128) void ikg_table_write_kernel(double* __restrict__ dst, int n, TableChunk c) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i < n) dst[i] = c.x[i];
}

hipError_t launch_table_write(double* dst, const double* host, size_t n, hipStream_t s) {
  for (size_t off = 0; off < n; off += kTableChunk) {
    TableChunk c;
    const int m = (int)std::min<size_t>(kTableChunk, n - off);
    std::memcpy(c.x, host + off, sizeof(double) * m);
    hipLaunchKernelGGL(ikg_table_write_kernel, dim3((m + 127) / 128), dim3(128), 0, s, dst + off, m, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// out[k, c] = curve(times[k])[c]: one lane per entry
__global__ __launch_bounds__(256) void ikg_bezier_eval_kernel(KBezier<double> c, const double* __restrict__ times,
                                                              int64_t K, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= K * c.dim) return;
  const int64_t k = i / c.dim;
  out[i] = bezier_eval(c, times[k], (int)(i % c.dim));
}

hipError_t launch_bezier_eval(const double* table, int n_points, int dim, double t_min, double t_max, double mult,
                              const double* times, int64_t K, double* out, hipStream_t s) {
  const KBezier<double> c{table, table + (size_t)n_points * dim, n_points, dim, t_min, t_max, mult};
  const int64_t rows = ((int64_t)1 << 30) / dim;  // per launch: at most 2^30 entries
  for (int64_t off = 0; off < K; off += rows) {
    const int64_t n = std::min(rows, K - off);
    hipLaunchKernelGGL(ikg_bezier_eval_kernel, dim3((unsigned)((n * dim + 255) / 256)), dim3(256), 0, s, c,
                       times + off, n, out + off * dim);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---------------------------------------------------------------- closed-loop rollout
// state rows <- the start, and the desired state of tick 0: one lane per (state, joint)
__global__ __launch_bounds__(256) void ikg_rollout_init_kernel(const double* __restrict__ q0,
                                                               const double* __restrict__ v0,
                                                               const double* __restrict__ t0, int nq, int64_t n,
                                                               StepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * nq) return;
  const int64_t p = i / nq;
  const int r = (int)(i % nq);
  const double t = t0 ? t0[p] : a.cv.q_tmin;
  ((double*)a.q)[i] = q0[i];
  ((double*)a.v)[i] = v0 ? v0[i] : 0.0;
  const bool ps = a.cv.stride_q != 0;
  const KBezier<double> cq = ps ? curve_q<true>(a.cv, a.cv.table, nq, p) : curve_q<false>(a.cv, a.cv.table, nq, p);
  const KBezier<double> cv = ps ? curve_v<true>(a.cv, a.cv.table, nq, p) : curve_v<false>(a.cv, a.cv.table, nq, p);
  ((double*)a.qdes)[i] = bezier_eval(cq, bezier_clamp(cq, t), r);
  ((double*)a.vdes)[i] = bezier_eval(cv, bezier_clamp(cv, t), r);
  if (r == 0) ((double*)a.t)[p] = t;
}

hipError_t launch_rollout_init(const void* q0, const void* v0, const void* t0, int nq, int64_t n, const StepArgs& a,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t nblocks = (n * nq + 255) / 256;
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ikg_rollout_init_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, (const double*)q0,
                     (const double*)v0, (const double*)t0, nq, n, a);
  return hipGetLastError();
}

// One tick after the frame-kinematics and dynamics kernels filled the scratch:
// the solve kernel's layout and phases (lane r = row r = joint r), then on the
// factor of M the solve left in LDS the forward dynamics qdd = M^-1 (tau - nle),
// the integrator, the trajectory clock, the desired state of the next tick
// (Horner over the curves' control points, staged in LDS behind the states'
// workspaces; with a curve pair per state only the binomial factors are staged
// and each state reads its own control points) and this tick's record.  Groups past the end of the batch work on
// the last state and store nothing.
template <int G, bool PS>
__global__ __launch_bounds__(64) void ikg_control_step_kernel(CtlIn in, int nq, int64_t B, KCtl<double> prm,
                                                              StepArgs a) {
  using T = double;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int grp = lane / G, r = lane % G;
  const int64_t p0 = (int64_t)blockIdx.x * (64 / G);
  const bool live = p0 + grp < B;
  const int64_t p = live ? p0 + grp : B - 1;
  T* base = reinterpret_cast<T*>(smem);
  CtlWs<T> w, f;
  ctl_ws_bind(base + (size_t)grp * step_ws_len(nq), nq, w);
  T* flag = base + (size_t)grp * step_ws_len(nq) + ctl_ws_len(nq);
  T* tab = base + (size_t)(64 / G) * step_ws_len(nq);
  const int ntab = (int)rollout_table_len(nq, a.cv.nq_pts, a.cv.nv_pts, PS);
  for (int i = lane; i < ntab; i += 64) tab[i] = a.cv.table[i];
  ctl_ws_load_lanes(w, in, p, r, G);
  const bool row = live && r < nq;
  T q = row ? ((const T*)a.q)[p * nq + r] : T(0);
  T v = row ? ((const T*)a.v)[p * nq + r] : T(0);
  const T t = ((const T*)a.t)[p] + a.dt_traj;
  __syncthreads();
  LaneRows<T> rows{r};
  control_solve_phases(w, prm, rows);
  const T tau = step_rhs(w, prm, flag, r);
  __syncthreads();
  fd_view(w, flag, f);
  ctl_substitute(f, rows);
  if (!live) return;
  if (r < nq) {
    step_integrate(a.dt_sim, f.qdd[r], q, v);
    ((T*)a.q)[p * nq + r] = q;
    ((T*)a.v)[p * nq + r] = v;
    const KBezier<T> cq = curve_q<PS>(a.cv, tab, nq, p), cv = curve_v<PS>(a.cv, tab, nq, p);
    ((T*)a.qdes)[p * nq + r] = bezier_eval(cq, bezier_clamp(cq, t), r);
    ((T*)a.vdes)[p * nq + r] = bezier_eval(cv, bezier_clamp(cv, t), r);
    if (a.slot >= 0) {
      const int64_t h = (p * a.R + a.slot) * nq + r;
      if (a.q_hist) ((T*)a.q_hist)[h] = q;
      if (a.v_hist) ((T*)a.v_hist)[h] = v;
      if (a.tau_hist) ((T*)a.tau_hist)[h] = tau;
    }
  }
  if (r == 0) ((T*)a.t)[p] = t;
}

namespace {

template <int G, bool PS>
hipError_t launch_step(unsigned nblocks, const CtlIn& in, int nq, int64_t B, const KCtl<double>& prm, const StepArgs& a,
                       hipStream_t s) {
  const size_t lds =
      sizeof(double) * ((64 / G) * step_ws_len(nq) + rollout_table_len(nq, a.cv.nq_pts, a.cv.nv_pts, PS));
  if (lds > 65536) {  // long curves on a wide model: above the default limit of dynamic LDS
    const hipError_t e = hipFuncSetAttribute((const void*)ikg_control_step_kernel<G, PS>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((ikg_control_step_kernel<G, PS>), dim3(nblocks), dim3(64), lds, s, in, nq, B, prm, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_control_step(const CtlIn& in, int nq, int64_t B, const KCtl<double>& prm, const StepArgs& a,
                               hipStream_t s) {
  return launch_per_state(nq, B, [&](auto g, unsigned nblocks) {
    constexpr int G = decltype(g)::value;
    return a.cv.stride_q != 0 ? launch_step<G, true>(nblocks, in, nq, B, prm, a, s)
                              : launch_step<G, false>(nblocks, in, nq, B, prm, a, s);
  });
}

// ---------------------------------------------------------------- inverse dynamics along curves
// ikg_trajectory_dynamics_batch: ikg_dynamics_kernel's layout (G lanes per
// sample, one lane per body, parents by ds_bpermute) over the samples of a
// curve.  One wave walks a.spw consecutive samples of one curve (block = curve *
// a.chunks + chunk), 64 / G side by side; the groups of a ragged last round
// repeat the run's last sample and store nothing.  The curve's control points
// and those of its two derivatives (Bezier.derivative, formed here once per
// wave) are staged in LDS; lane j does the Horner for joint j's q, qd, qdd, the
// forward rounds with the acceleration included (dyn_forward_acc), both forces,
// the subtree sums over j ascending, tau_j = S_j . fc and g_j = S_j . gc.  A lane
// folds its own joint over the run, a butterfly folds the lanes (peak_merge does
// not depend on the order), lane 0 writes the run's partial; the second kernel
// folds the runs per curve.
namespace {

__device__ inline void peak_fold_lanes(DynPeak& p) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    DynPeak o;
    o.val = __shfl_xor(p.val, off, 64);
    o.sample = __shfl_xor(p.sample, off, 64);
    o.joint = __shfl_xor(p.joint, off, 64);
    peak_merge(p, o);
  }
}

}  // namespace

template <int G>
__global__ __launch_bounds__(64) void ikg_trajdyn_kernel(const KModel<double>* __restrict__ m,
                                                         const KInertia<double>* __restrict__ in,
                                                         const TrajDynArgs a) {
  using T = double;
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int kSide = 64 / G;
  const int nq = m->nq, n = a.n_points;
  T* Pq = reinterpret_cast<T*>(smem);
  T* Pv = Pq + n * nq;
  T* Pa = Pv + (n - 1) * nq;
  const int lane = threadIdx.x;
  const int grp = lane / G, b = lane % G, gbase = grp * G;
  const int64_t curve = blockIdx.x / a.chunks;
  const int ch = (int)(blockIdx.x % a.chunks);
  const int k0 = ch * a.spw, k1 = min(a.S, k0 + a.spw);
  const T* gp = a.points + curve * n * nq;
  for (int i = lane; i < n * nq; i += 64) Pq[i] = gp[i];
  __syncthreads();
  for (int i = lane; i < (n - 1) * nq; i += 64) Pv[i] = bezier_derivative_point(Pq, n, nq, i / nq, i % nq);
  __syncthreads();
  for (int i = lane; i < (n - 2) * nq; i += 64) Pa[i] = bezier_derivative_point(Pv, n - 1, nq, i / nq, i % nq);
  __syncthreads();
  const KBezier<T> cq{Pq, a.bc[0], n, nq, a.t_min, a.t_max, a.mult};
  const KBezier<T> cv{Pv, a.bc[1], n - 1, nq, a.t_min, a.t_max, a.mult_v};
  const KBezier<T> ca{Pa, a.bc[2], n - 2, nq, a.t_min, a.t_max, a.mult_a};
  // this lane's joint and body (idle lanes: a massless joint under the universe)
  const bool body = b < nq;
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
  const T grav[3] = {in->grav[0], in->grav[1], in->grav[2]};
  const T ref[3] = {in->ref[0], in->ref[1], in->ref[2]};
  const int levels = in->levels;
  const T vlim = a.vlim[bi], elim = a.elim[bi];
  const int src = parent >= 0 ? gbase + parent : lane;
  DynBody<T> uni;
  dyn_universe(grav, ref, uni);
  const T zero[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  TrajDynPartial part;
  dynpartial_init(part);
#pragma unroll 1
  for (int kb = k0; kb < k1; kb += kSide) {
    const bool on = kb + grp < k1;
    const int k = on ? kb + grp : k1 - 1;
    const T t = trajcheck_time(a.t_min, a.t_max, a.S, k);
    const T q = body ? bezier_eval(cq, t, b) : T(0);
    const T qd = body ? bezier_eval(cv, t, b) : T(0);
    const T qdd = body ? bezier_eval(ca, t, b) : T(0);
    T s, c;
    cw_sincos(q, &s, &c);
    DynBody<T> me = uni;
    T S[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
#pragma unroll 1
    for (int l = 0; l < levels; ++l) {
      DynBody<T> par;
      lane_get_n(me.R, src, par.R);
      lane_get_n(me.o, src, par.o);
      lane_get_n(me.v, src, par.v);
      lane_get_n(me.a, src, par.a);
      if (parent < 0) par = uni;
      dyn_forward_acc(par, jR, jt, axis, s, c, qd, qdd, me, S);
    }
    DynInertia<T> W;
    dyn_inertia_world(mass, h, Io, me.R, me.o, W);
    T f[6], f0[6];
    dyn_force(W, me.v, me.a, f);
    dyn_force(W, zero, uni.a, f0);
    T fc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, gc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
#pragma unroll 1
    for (int j = 0; j < nq; ++j) {
      const bool mine = (in->anc[j] >> b) & 1;  // j in the subtree of b
      T fj[6], gj[6];
      lane_get_n(f, gbase + j, fj);
      lane_get_n(f0, gbase + j, gj);
      if (mine) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          fc[i] += fj[i];
          gc[i] += gj[i];
        }
      }
    }
    const T tau = ddot6(S, fc), g = ddot6(S, gc);
    if (on && body) {
      dynpartial_add(part, k, b, qd, tau, g, vlim, elim);
      const int64_t at = (curve * a.S + k) * nq + b;
      if (a.tau) a.tau[at] = tau;
      if (a.g) a.g[at] = g;
    }
  }
  peak_fold_lanes(part.speed);
  peak_fold_lanes(part.torque_use);
  peak_fold_lanes(part.static_use);
  peak_fold_lanes(part.torque_scale);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part.n_static += __shfl_xor(part.n_static, off, 64);
  if (lane == 0) a.part[blockIdx.x] = part;
}

// The runs' partials of each curve folded in sample order, one lane per curve.
__global__ __launch_bounds__(256) void ikg_trajdyn_fold_kernel(const TrajDynPartial* __restrict__ part, int chunks,
                                                               int64_t B, const TrajDynFoldOut o) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  TrajDynPartial acc = part[b * chunks];
  for (int ch = 1; ch < chunks; ++ch) dynpartial_merge(acc, part[b * chunks + ch]);
  dynfold_store(o, b, acc);
}

hipError_t launch_trajdyn(const KModel<double>* dm, const KInertia<double>* di, int nq, const TrajDynArgs& a, int64_t B,
                          const TrajDynFoldOut& o, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const size_t lds = sizeof(double) * (size_t)(3 * a.n_points - 3) * nq;
  const unsigned nblocks = (unsigned)(B * a.chunks);
  if (nq <= 16)
    hipLaunchKernelGGL((ikg_trajdyn_kernel<16>), dim3(nblocks), dim3(64), lds, s, dm, di, a);
  else
    hipLaunchKernelGGL((ikg_trajdyn_kernel<32>), dim3(nblocks), dim3(64), lds, s, dm, di, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ikg_trajdyn_fold_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, a.part, a.chunks, B,
                     o);
  return hipGetLastError();
}

template hipError_t launch_dynamics<double>(const KModel<double>*, const KInertia<double>*, int, const void*,
                                            const void*, int64_t, const DynOut&, hipStream_t);
template hipError_t launch_dynamics<float>(const KModel<float>*, const KInertia<float>*, int, const void*,
                                           const void*, int64_t, const DynOut&, hipStream_t);

}  // namespace ikg
