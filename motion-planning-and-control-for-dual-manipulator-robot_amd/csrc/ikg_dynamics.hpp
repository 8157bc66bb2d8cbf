// Controller dynamics (control.py:284-286): the joint-space inertia matrix M
// (pin.computeAllTerms -> data.M) and the non-linear effects b
// (pin.nonLinearEffects) of a joint tree, as per-body __host__ __device__
// functions shared by the kernel (ikg_dynamics.hip) and the host emulator
// (ikg_host_emu.hip).
//
// Formulation: spatial algebra in ONE frame, the world frame with the world
// origin as reference point.  A motion is [v_O; w] (v_O = velocity of the body
// point that coincides with the world origin), a force [f; n_O].  In that frame
//   * a revolute joint's motion subspace is S_i = [o_i x a_i; a_i]
//     (a_i world axis, o_i world origin of the joint);
//   * rigid-body inertias need no transport between bodies: the composite
//     inertia of a subtree is the plain sum of its bodies' world inertias, and
//     the force on a subtree the plain sum of its bodies' forces;
//   * composite-rigid-body:  M_ij = S_j . (Ic_i S_i)  for j = i or an ancestor of i;
//   * recursive Newton-Euler at zero joint acceleration:
//       v_i = v_p + S_i qd_i,  a_i = a_p + (v_i x S_i) qd_i,  a_universe = [-gravity; 0],
//       f_i = I_i a_i + v_i x* (I_i v_i),  nle_i = S_i . sum_{j in subtree(i)} f_j;
//     g is the same sum with v = 0 (f_j = I_j a_universe), so nle == g to the
//     bit when every joint velocity is zero.
// Any fixed reference point serves as "the world origin" above; M and nle do
// not depend on it, but the rounding does: the inertias about the point carry
// m |o|^2 terms that cancel in M.  The tables therefore name a point in the
// middle of the robot (KInertia::ref, the centroid of the joint origins at
// q = 0) and every origin is taken relative to it (measured in fp32 on the
// Nextage: max error of M 1.9e-6 of max|M| about the world origin).
// A rigid-body inertia about the reference point is (m, h = m c, I_O [6]); the
// model tables hold each body's (m, m c, I about the joint origin) in its joint
// frame, pre-combined on the host in fp64 (build_kinertia).
#pragma once

#include <cmath>
#include <cstring>

#include "ikg_device.hpp"
#include "ikgrasp.h"

namespace ikg {

template <typename T>
struct KInertia {
  T mass[kMaxNq];
  T h[kMaxNq][3];    // first moment m c, joint frame
  T Io[kMaxNq][6];   // xx xy xz yy yz zz about the joint origin, joint-frame axes
  T grav[3];         // world frame
  T ref[3];          // reference point of the spatial quantities (world frame, see below)
  uint32_t anc[kMaxNq];  // bit j: joint j is joint i itself or one of its ancestors
  int32_t levels;        // joints on the longest root-to-leaf chain
};

// fp64 pre-combination of the descriptor's (mass, com, inertia about the com)
inline void body_at_joint_origin(const ikg_inertia_desc& d, int i, double* h, double* Io) {
  const double m = d.mass[i];
  const double* c = d.com[i];
  const double* I = d.inertia[i];
  const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  for (int k = 0; k < 3; ++k) h[k] = m * c[k];
  Io[0] = I[0] + m * (cc - c[0] * c[0]);
  Io[1] = I[1] - m * c[0] * c[1];
  Io[2] = I[2] - m * c[0] * c[2];
  Io[3] = I[3] + m * (cc - c[1] * c[1]);
  Io[4] = I[4] - m * c[1] * c[2];
  Io[5] = I[5] + m * (cc - c[2] * c[2]);
}

template <typename T>
inline void build_kinertia(const ikg_model_desc& md, const ikg_inertia_desc& d, KInertia<T>& k) {
  std::memset(&k, 0, sizeof(k));
  int levels = 0;
  for (int i = 0; i < md.nq; ++i) {
    double h[3], Io[6];
    body_at_joint_origin(d, i, h, Io);
    k.mass[i] = (T)d.mass[i];
    for (int j = 0; j < 3; ++j) k.h[i][j] = (T)h[j];
    for (int j = 0; j < 6; ++j) k.Io[i][j] = (T)Io[j];
    uint32_t a = 0;
    int depth = 0;
    for (int j = i; j >= 0; j = md.parent[j]) {
      a |= 1u << j;
      ++depth;
    }
    k.anc[i] = a;
    if (depth > levels) levels = depth;
  }
  for (int j = 0; j < 3; ++j) k.grav[j] = (T)d.gravity[j];
  k.levels = levels;
  // reference point: the centroid of the joint origins at q = 0 (fp64 FK of the placements)
  double R[IKG_MAX_NQ][9], o[IKG_MAX_NQ][3], ref[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < md.nq; ++i) {
    const double* P = md.placement[i];
    const int p = md.parent[i];
    for (int r = 0; r < 3; ++r) {
      o[i][r] = p >= 0 ? o[p][r] + R[p][3 * r] * P[9] + R[p][3 * r + 1] * P[10] + R[p][3 * r + 2] * P[11] : P[9 + r];
      for (int c = 0; c < 3; ++c)
        R[i][3 * r + c] = p >= 0 ? R[p][3 * r] * P[c] + R[p][3 * r + 1] * P[3 + c] + R[p][3 * r + 2] * P[6 + c]
                                 : P[3 * r + c];
      ref[r] += o[i][r] / md.nq;
    }
  }
  for (int j = 0; j < 3; ++j) k.ref[j] = (T)ref[j];
}

// mass >= 0, finite entries, inertia about the com positive semi-definite with
// principal moments obeying the triangle inequalities (tr I >= 2 lambda_max,
// i.e. (tr I / 2) 1 - I positive semi-definite).  Returns the offending body
// and sets *why, or -1.
inline bool psd3(const double* s, double tol) {  // xx xy xz yy yz zz
  const double a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5];
  const double m1 = a * d - b * b, m2 = a * f - c * c, m3 = d * f - e * e;
  const double det = a * m3 - b * (b * f - c * e) + c * (b * e - c * d);
  return a >= -tol && d >= -tol && f >= -tol && m1 >= -tol * tol && m2 >= -tol * tol && m3 >= -tol * tol &&
         det >= -tol * tol * tol;
}

inline int check_inertia_desc(const ikg_inertia_desc& d, int nq, const char** why) {
  for (int j = 0; j < 3; ++j)
    if (!std::isfinite(d.gravity[j])) {
      *why = "gravity is not finite";
      return nq;
    }
  for (int i = 0; i < nq; ++i) {
    bool fin = std::isfinite(d.mass[i]);
    for (int j = 0; j < 3; ++j) fin = fin && std::isfinite(d.com[i][j]);
    for (int j = 0; j < 6; ++j) fin = fin && std::isfinite(d.inertia[i][j]);
    if (!fin) {
      *why = "non-finite entry";
      return i;
    }
    if (d.mass[i] < 0) {
      *why = "negative mass";
      return i;
    }
    const double* I = d.inertia[i];
    const double scale = std::fabs(I[0]) + std::fabs(I[3]) + std::fabs(I[5]) + std::fabs(I[1]) + std::fabs(I[2]) +
                         std::fabs(I[4]);
    const double tol = 1e-9 * (scale > 1e-300 ? scale : 1e-300);
    if (!psd3(I, tol)) {
      *why = "inertia is not positive semi-definite";
      return i;
    }
    const double ht = 0.5 * (I[0] + I[3] + I[5]);
    const double tri[6] = {ht - I[0], -I[1], -I[2], ht - I[3], -I[4], ht - I[5]};
    if (!psd3(tri, tol)) {
      *why = "principal moments violate the triangle inequality";
      return i;
    }
  }
  return -1;
}

// ---------------------------------------------------------------- per-body device math
template <typename T>
IKG_HD inline void dcross(const T* a, const T* b, T* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

template <typename T>
IKG_HD inline T ddot6(const T* a, const T* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}

// world placement of a joint frame, the spatial velocity and acceleration of
// its body (world frame, world origin)
template <typename T>
struct DynBody {
  T R[9], o[3], v[6], a[6];
};

// world-frame rigid-body inertia about the world origin
template <typename T>
struct DynInertia {
  T m, h[3], I[6];
};

// the universe as a joint's parent, seen from the reference point: a_universe = [-gravity; 0]
template <typename T>
IKG_HD inline void dyn_universe(const T* grav, const T* ref, DynBody<T>& b) {
#pragma unroll
  for (int i = 0; i < 9; ++i) b.R[i] = T(i % 4 == 0);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    b.o[i] = -ref[i];
    b.v[i] = b.v[3 + i] = T(0);
    b.a[i] = -grav[i];
    b.a[3 + i] = T(0);
  }
}

// Body i from its parent: placement (jR, jt) then the joint rotation about the
// canonical axis (runtime index: the branch-free one-hot form of
// ikg_control.hip col_rot, R Rot = c R + s R [e]x + (1 - c)(R e) e^T), joint
// rate qd.  Out: the body state and its motion subspace S = [o x a; a].
template <typename T>
IKG_HD inline void dyn_forward(const DynBody<T>& par, const T* jR, const T* jt, int axis, T s, T c, T qd,
                               DynBody<T>& b, T* S) {
  T P[9], d[3], ax[3];
  matmul3(par.R, jR, P);
  matvec3(par.R, jt, d);
  const T e0 = T(axis == 0), e1 = T(axis == 1), e2 = T(axis == 2);
  const T omc = T(1) - c;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const T r0 = P[3 * r], r1 = P[3 * r + 1], r2 = P[3 * r + 2];
    const T u = e0 * r0 + e1 * r1 + e2 * r2;
    ax[r] = u;
    b.R[3 * r + 0] = c * r0 + s * (e2 * r1 - e1 * r2) + omc * u * e0;
    b.R[3 * r + 1] = c * r1 + s * (e0 * r2 - e2 * r0) + omc * u * e1;
    b.R[3 * r + 2] = c * r2 + s * (e1 * r0 - e0 * r1) + omc * u * e2;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) b.o[i] = par.o[i] + d[i];
  dcross(b.o, ax, S);
#pragma unroll
  for (int i = 0; i < 3; ++i) S[3 + i] = ax[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) b.v[i] = par.v[i] + S[i] * qd;
  // dS/dt = v x S (motion cross product): [w x S_lin + v_lin x S_ang; w x S_ang]
  T t1[3], t2[3], t3[3];
  dcross(b.v + 3, S, t1);
  dcross(b.v, S + 3, t2);
  dcross(b.v + 3, S + 3, t3);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    b.a[i] = par.a[i] + (t1[i] + t2[i]) * qd;
    b.a[3 + i] = par.a[3 + i] + t3[i] * qd;
  }
}

// (m, h, Io) in the joint frame at the joint origin -> world axes, world origin:
//   h_W = R h + m o,   I_W = R Io R^T + m (|o|^2 1 - o o^T) + 2 (o . Rh) 1 - o (Rh)^T - (Rh) o^T
template <typename T>
IKG_HD inline void dyn_inertia_world(T m, const T* h, const T* Io, const T* R, const T* o, DynInertia<T>& W) {
  T hd[3], A[9], B[9];
  matvec3(R, h, hd);
  const T I9[9] = {Io[0], Io[1], Io[2], Io[1], Io[3], Io[4], Io[2], Io[4], Io[5]};
  matmul3(R, I9, A);
  matmul3_nt(A, R, B);
  const T oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2];
  const T oh = o[0] * hd[0] + o[1] * hd[1] + o[2] * hd[2];
  const T dg = m * oo + T(2) * oh;
  W.m = m;
#pragma unroll
  for (int i = 0; i < 3; ++i) W.h[i] = hd[i] + m * o[i];
  W.I[0] = B[0] + dg - m * o[0] * o[0] - T(2) * o[0] * hd[0];
  W.I[1] = B[1] - m * o[0] * o[1] - o[0] * hd[1] - hd[0] * o[1];
  W.I[2] = B[2] - m * o[0] * o[2] - o[0] * hd[2] - hd[0] * o[2];
  W.I[3] = B[4] + dg - m * o[1] * o[1] - T(2) * o[1] * hd[1];
  W.I[4] = B[5] - m * o[1] * o[2] - o[1] * hd[2] - hd[1] * o[2];
  W.I[5] = B[8] + dg - m * o[2] * o[2] - T(2) * o[2] * hd[2];
}

// I x for a motion x = [v; w]:  [m v + w x h;  h x v + I w]
template <typename T>
IKG_HD inline void dyn_apply(const DynInertia<T>& W, const T* x, T* out) {
  T wh[3], hv[3];
  dcross(x + 3, W.h, wh);
  dcross(W.h, x, hv);
  const T* w = x + 3;
  out[0] = W.m * x[0] + wh[0];
  out[1] = W.m * x[1] + wh[1];
  out[2] = W.m * x[2] + wh[2];
  out[3] = hv[0] + (W.I[0] * w[0] + W.I[1] * w[1] + W.I[2] * w[2]);
  out[4] = hv[1] + (W.I[1] * w[0] + W.I[3] * w[1] + W.I[4] * w[2]);
  out[5] = hv[2] + (W.I[2] * w[0] + W.I[4] * w[1] + W.I[5] * w[2]);
}

// f = I a + v x* (I v),  v x* [p; l] = [w x p;  w x l + v_lin x p]
template <typename T>
IKG_HD inline void dyn_force(const DynInertia<T>& W, const T* v, const T* a, T* f) {
  T Ia[6], Iv[6], t1[3], t2[3], t3[3];
  dyn_apply(W, a, Ia);
  dyn_apply(W, v, Iv);
  dcross(v + 3, Iv, t1);
  dcross(v + 3, Iv + 3, t2);
  dcross(v, Iv, t3);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f[i] = Ia[i] + t1[i];
    f[3 + i] = Ia[3 + i] + (t2[i] + t3[i]);
  }
}

template <typename T>
IKG_HD inline void dyn_inertia_zero(DynInertia<T>& W) {
  W.m = T(0);
#pragma unroll
  for (int i = 0; i < 3; ++i) W.h[i] = T(0);
#pragma unroll
  for (int i = 0; i < 6; ++i) W.I[i] = T(0);
}

template <typename T>
IKG_HD inline void dyn_inertia_add(DynInertia<T>& A, const DynInertia<T>& B) {
  A.m += B.m;
#pragma unroll
  for (int i = 0; i < 3; ++i) A.h[i] += B.h[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) A.I[i] += B.I[i];
}

// The forward pass of one state on the host, parents before children: the
// universe, every body's state and motion subspace (v null: zero velocity)
template <typename T>
inline void forward_bodies(const KModel<T>& m, const KInertia<T>& in, const T* q, const T* v, DynBody<T>& uni,
                           DynBody<T>* body, T (*S)[6]) {
  dyn_universe(in.grav, in.ref, uni);
  for (int i = 0; i < m.nq; ++i) {
    T s, c;
    cw_sincos(q[i], &s, &c);
    const DynBody<T>& par = m.jparent[i] >= 0 ? body[m.jparent[i]] : uni;
    dyn_forward(par, m.jR[i], m.jt[i], m.jaxis[i], s, c, v ? v[i] : T(0), body[i], S[i]);
  }
}

// One state on the host, body by body in the order the kernel's lane group
// works (ikg_dynamics.hip): forward pass, subtree sums over j ascending, then
// the rows of M.  M [nq,nq], nle [nq], g [nq]; any may be null.
template <typename T>
inline void dynamics_state(const KModel<T>& m, const KInertia<T>& in, const T* q, const T* v, T* M, T* nle, T* g) {
  const int nq = m.nq;
  DynBody<T> body[kMaxNq];
  DynInertia<T> W[kMaxNq];
  T S[kMaxNq][6], f[kMaxNq][6], f0[kMaxNq][6];
  DynBody<T> uni;
  forward_bodies(m, in, q, v, uni, body, S);
  for (int i = 0; i < nq; ++i) {
    dyn_inertia_world(in.mass[i], in.h[i], in.Io[i], body[i].R, body[i].o, W[i]);
    dyn_force(W[i], body[i].v, body[i].a, f[i]);
    const T zero[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    dyn_force(W[i], zero, uni.a, f0[i]);
  }
  if (M)
    for (int i = 0; i < nq * nq; ++i) M[i] = T(0);
  for (int i = 0; i < nq; ++i) {
    DynInertia<T> Ic;
    dyn_inertia_zero(Ic);
    T fc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, gc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    for (int j = 0; j < nq; ++j)
      if ((in.anc[j] >> i) & 1) {  // j in the subtree of i
        dyn_inertia_add(Ic, W[j]);
        for (int k = 0; k < 6; ++k) {
          fc[k] += f[j][k];
          gc[k] += f0[j][k];
        }
      }
    if (nle) nle[i] = ddot6(S[i], fc);
    if (g) g[i] = ddot6(S[i], gc);
    if (M) {
      T F[6];
      dyn_apply(Ic, S[i], F);
      for (int j = 0; j < nq; ++j)
        if ((in.anc[i] >> j) & 1) {
          const T x = ddot6(S[j], F);
          M[i * nq + j] = x;
          M[j * nq + i] = x;
        }
    }
  }
}

// ---------------------------------------------------------------- M about each joint's own origin
// Forward dynamics divides by M, so it needs the SMALL entries of M (the wrist
// rows, 1e-4 of max|M|) to their own relative accuracy.  About one common
// reference point every body's inertia carries m |o|^2 terms that cancel in
// those entries: M above is within 4e-16 of max|M|, an absolute error the wrist
// rows see in full, and cond(M) ~ 1e4 carries it into qdd (measured 1.8e-13 of
// max|qdd| against 2e-15 for a body-local M).  So row i is formed about joint
// i's own origin o_i, where only distances inside the subtree of i appear:
//   Ic_i = sum_{j in subtree(i)} inertia of body j about o_i   (dyn_inertia_world with o = o_j - o_i)
//   F_i  = Ic_i [0; a_i],   M_ij = [(o_j - o_i) x a_j; a_j] . F_i   for j = i or an ancestor of i.
// motion subspace of joint j (origin oj, world axis aj) about the point oi
template <typename T>
IKG_HD inline void dyn_subspace_about(const T* oj, const T* oi, const T* aj, T* S) {
  const T d[3] = {oj[0] - oi[0], oj[1] - oi[1], oj[2] - oi[2]};
  dcross(d, aj, S);
#pragma unroll
  for (int i = 0; i < 3; ++i) S[3 + i] = aj[i];
}

// body j (placement Rj, oj) as seen from the point oi, added to Ic
template <typename T>
IKG_HD inline void dyn_inertia_add_about(T m, const T* h, const T* Io, const T* Rj, const T* oj, const T* oi,
                                         DynInertia<T>& Ic) {
  const T d[3] = {oj[0] - oi[0], oj[1] - oi[1], oj[2] - oi[2]};
  DynInertia<T> W;
  dyn_inertia_world(m, h, Io, Rj, d, W);
  dyn_inertia_add(Ic, W);
}

// One state on the host, in the forward-dynamics kernel's order: M [nq,nq], both triangles
template <typename T>
inline void inertia_matrix_local_state(const KModel<T>& m, const KInertia<T>& in, const T* q, T* M) {
  const int nq = m.nq;
  DynBody<T> body[kMaxNq];
  T S[kMaxNq][6];
  DynBody<T> uni;
  forward_bodies(m, in, q, (const T*)nullptr, uni, body, S);
  for (int i = 0; i < nq * nq; ++i) M[i] = T(0);
  for (int i = 0; i < nq; ++i) {
    DynInertia<T> Ic;
    dyn_inertia_zero(Ic);
    for (int j = 0; j < nq; ++j)
      if ((in.anc[j] >> i) & 1) dyn_inertia_add_about(in.mass[j], in.h[j], in.Io[j], body[j].R, body[j].o, body[i].o, Ic);
    T Si[6], F[6];
    dyn_subspace_about(body[i].o, body[i].o, S[i] + 3, Si);
    dyn_apply(Ic, Si, F);
    for (int j = 0; j < nq; ++j)
      if ((in.anc[i] >> j) & 1) {
        T Sj[6];
        dyn_subspace_about(body[j].o, body[i].o, S[j] + 3, Sj);
        const T x = ddot6(Sj, F);
        M[i * nq + j] = x;
        M[j * nq + i] = x;
      }
  }
}

// ---------------------------------------------------------------- controller solve (control.py:348-406)
// Per state, from M, nle (above) and the kinematic terms J [12,nq], dJ v, e,
// e' of ikg_frame_kinematics_batch (LOCAL_WORLD_ALIGNED):
//   Lambda_h = (J_h M^-1 J_h^T + lambda_reg 1)^-1                    (:348-349)
//   fc_h = [Kf e_t; Kt e_r],  xdd_h = Kp e + Kv e' + Lambda_h fc_h  (:338-360)
//   qdd = (J^T J + qp_reg 1)^-1 J^T (xdd - dJ v)                    (:381-395; quadprog without constraints)
//   tau = M qdd + nle + J^T (fc + fc_bias), zero_tau_mask entries 0 (:401-406)
// Every inverse is a square-root-free Cholesky factorisation A = L D L^T of a
// symmetric positive definite matrix (M; J M^-1 J^T + lambda 1; J^T J + reg 1,
// smallest eigenvalue >= reg), done in place in the lower triangle: after
// step k column k holds w_rk = l_rk d_k and the diagonal d_k, and the upper
// triangle keeps the original matrix (tau needs M itself).
//
// The work of a state is written as PHASES over a row index r: phase(ws, r)
// touches only row r's share, and all rows of one phase are independent.  The
// kernel runs a phase with one lane per row and a barrier between phases; the
// host emulator runs the same functions in a loop over r.
template <typename T>
struct KCtl {
  T Kp, Kv, Kf, Kt, lambda_reg, qp_reg;
  T fc_bias[12];
  uint32_t zero_tau_mask;
};

template <typename T>
inline KCtl<T> make_kctl(const ikg_control_params& p) {
  KCtl<T> k;
  k.Kp = (T)p.Kp;
  k.Kv = (T)p.Kv;
  k.Kf = (T)p.Kf;
  k.Kt = (T)p.Kt;
  k.lambda_reg = (T)p.lambda_reg;
  k.qp_reg = (T)p.qp_reg;
  for (int i = 0; i < 12; ++i) k.fc_bias[i] = (T)p.fc_bias[i];
  k.zero_tau_mask = p.zero_tau_mask;
  return k;
}

// a state's workspace (LDS in the kernel): row stride ld = nq | 1 (odd, so
// lanes that walk different rows hit different banks)
template <typename T>
struct CtlWs {
  int nq, ld;
  T *M, *Md, *Mr, *Ms;  // [nq*ld]; the original diagonal of M; 1 / d_k and sqrt(d_k) of its factorisation
  T *J, *Z;             // [12*ld] J[k*ld + r];  Z[c*ld + i] = (L^-1 J^T)_ic / sqrt(d_i)
  T *H;                 // [nq*ld] J^T J + reg 1 and its factorisation
  T *A;                 // [2][6*7] J_h M^-1 J_h^T + lambda 1 and its factorisation
  T *nle, *rhs, *qdd;   // [nq]
  T *e, *ed, *dJv, *fc, *xdd;  // [12]
  T *fail;              // [1] != 0: a pivot of H was not positive
};

IKG_HD inline int ctl_ws_len(int nq) {
  const int ld = nq | 1;
  return 2 * nq * ld + 24 * ld + 6 * nq + 84 + 60 + 2;
}

template <typename T>
IKG_HD inline void ctl_ws_bind(T* base, int nq, CtlWs<T>& w) {
  const int ld = nq | 1;
  w.nq = nq;
  w.ld = ld;
  T* p = base;
  w.M = p, p += nq * ld;
  w.H = p, p += nq * ld;
  w.J = p, p += 12 * ld;
  w.Z = p, p += 12 * ld;
  w.Md = p, p += nq;
  w.Mr = p, p += nq;
  w.Ms = p, p += nq;
  w.nle = p, p += nq;
  w.rhs = p, p += nq;
  w.qdd = p, p += nq;
  w.A = p, p += 84;
  w.e = p, p += 12;
  w.ed = p, p += 12;
  w.dJv = p, p += 12;
  w.fc = p, p += 12;
  w.xdd = p, p += 12;
  w.fail = p;
}

// step k of the in-place L D L^T of the n x n matrix A (row stride ld), row r
template <typename T>
IKG_HD inline void ldl_step(T* A, int ld, int n, int k, int r) {
  if (r > k && r < n) {
    const T t = A[r * ld + k] / A[k * ld + k];
    for (int c = k + 1; c <= r; ++c) A[r * ld + c] -= t * A[c * ld + k];
  }
}

template <typename T>
IKG_HD inline void ctl_pivots(const CtlWs<T>& w, int r) {
  if (r < w.nq) {
    const T d = w.M[r * w.ld + r];
    w.Mr[r] = T(1) / d;
    w.Ms[r] = ::sqrt(d);
  }
  if (r == 0) *w.fail = T(0);
}

// row c of J (c < 12): Z_c = D^-1/2 L^-1 J_c^T by forward substitution, and fc (:352-354)
template <typename T>
IKG_HD inline void ctl_forward(const CtlWs<T>& w, const KCtl<T>& p, int c) {
  if (c >= 12) return;
  w.fc[c] = ((c % 6) < 3 ? p.Kf : p.Kt) * w.e[c];
  T* z = w.Z + c * w.ld;
  for (int i = 0; i < w.nq; ++i) {
    T y = w.J[c * w.ld + i];
    for (int k = 0; k < i; ++k) y -= w.M[i * w.ld + k] * z[k];  // z[k] = y_k / d_k
    z[i] = y * w.Mr[i];
  }
  for (int i = 0; i < w.nq; ++i) z[i] *= w.Ms[i];
}

// row a of hand h's J_h M^-1 J_h^T + lambda 1 (:348-349), c = 6 h + a
template <typename T>
IKG_HD inline void ctl_opspace(const CtlWs<T>& w, const KCtl<T>& p, int c) {
  if (c >= 12) return;
  const int h = c / 6, a = c % 6;
  for (int b = 0; b < 6; ++b) {
    const T *za = w.Z + c * w.ld, *zb = w.Z + (6 * h + b) * w.ld;
    T acc = T(0);
    for (int i = 0; i < w.nq; ++i) acc += za[i] * zb[i];
    w.A[h * 42 + a * 7 + b] = acc + (a == b ? p.lambda_reg : T(0));
  }
}

template <typename T>
IKG_HD inline void ctl_opspace_step(const CtlWs<T>& w, int k, int c) {
  if (c < 12) ldl_step(w.A + (c / 6) * 42, 7, 6, k, c % 6);
}

// column (= row) a of Lambda_h = A^-1 and xdd (:338, :357-360), c = 6 h + a; Lambda row -> lam[6]
template <typename T>
IKG_HD inline void ctl_lambda(const CtlWs<T>& w, const KCtl<T>& p, int c, T* lam) {
  if (c >= 12) return;
  const int h = c / 6, a = c % 6;
  const T* A = w.A + h * 42;
  T y[6], u[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    T t = T(i == a);
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (k < i) t -= A[i * 7 + k] * u[k];
    y[i] = t;
    u[i] = t / A[i * 7 + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    T t = y[i];
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (k > i) t -= A[k * 7 + i] * lam[k];
    lam[i] = t / A[i * 7 + i];
  }
  T acc = T(0);
#pragma unroll
  for (int b = 0; b < 6; ++b) acc += lam[b] * w.fc[6 * h + b];
  w.xdd[c] = p.Kp * w.e[c] + p.Kv * w.ed[c] + acc;
}

// row r of H = J^T J + reg 1 (lower triangle) and of d = J^T (xdd - dJ v) (:381-387)
template <typename T>
IKG_HD inline void ctl_normal(const CtlWs<T>& w, const KCtl<T>& p, int r) {
  if (r >= w.nq) return;
  for (int c = 0; c <= r; ++c) {
    T acc = T(0);
    for (int k = 0; k < 12; ++k) acc += w.J[k * w.ld + r] * w.J[k * w.ld + c];
    w.H[r * w.ld + c] = acc + (c == r ? p.qp_reg : T(0));
  }
  T acc = T(0);
  for (int k = 0; k < 12; ++k) acc += w.J[k * w.ld + r] * (w.xdd[k] - w.dJv[k]);
  w.rhs[r] = acc;
}

template <typename T>
IKG_HD inline void ctl_check(const CtlWs<T>& w, int r) {
  if (r < w.nq && !(w.H[r * w.ld + r] > T(0))) *w.fail = T(1);
}

// L y = d, column k: y_k is final, rows r > k take its share
template <typename T>
IKG_HD inline void ctl_solve_fwd(const CtlWs<T>& w, int k, int r) {
  if (r > k && r < w.nq) w.rhs[r] -= w.H[r * w.ld + k] * (w.rhs[k] / w.H[k * w.ld + k]);
}

// D L^T x = y from the last row up: x_k = y_k / d_k, rows r < k take its share
template <typename T>
IKG_HD inline void ctl_solve_bwd(const CtlWs<T>& w, int k, int r) {
  const T xk = w.rhs[k] / w.H[k * w.ld + k];
  if (r == k) w.qdd[k] = (*w.fail != T(0)) ? T(0) : xk;
  if (r < k) w.rhs[r] -= w.H[k * w.ld + r] * xk;
}

// tau_r (:401-406)
template <typename T>
IKG_HD inline T ctl_tau(const CtlWs<T>& w, const KCtl<T>& p, int r) {
  T acc = T(0);
  for (int c = 0; c < w.nq; ++c) {
    const T m = c < r ? w.M[c * w.ld + r] : (c == r ? w.Md[r] : w.M[r * w.ld + c]);
    acc += m * w.qdd[c];
  }
  acc += w.nle[r];
  T jf = T(0);
  for (int k = 0; k < 12; ++k) jf += w.J[k * w.ld + r] * (w.fc[k] + p.fc_bias[k]);
  acc += jf;
  return ((p.zero_tau_mask >> r) & 1u) ? T(0) : acc;
}

// The phases in order, written once over an executor `rows`: rows(fn) runs
// fn(r) for the rows the caller owns and then makes their writes visible to all
// rows.  The kernel's executor is one lane per row and a barrier
// (ikg_dynamics.hip LaneRows); the host's is a loop over r (HostRows below).
// rows.lam(r) is where row r < 12 keeps its row of Lambda.
template <typename T>
struct HostRows {
  int R;      // rows of a phase
  T* Lambda;  // [2,36] or null
  T spare[6];
  template <typename F>
  void operator()(F&& fn) {
    for (int r = 0; r < R; ++r) fn(r);
  }
  T* lam(int r) { return Lambda && r < 12 ? Lambda + 6 * r : spare; }
};

// the in-place L D L^T of the n x n matrix A, a phase per column
template <typename T, typename Rows>
IKG_HD inline void ldl_factor(T* A, int ld, int n, Rows& rows) {
#pragma unroll 1
  for (int k = 0; k < n; ++k) rows([&](int r) { ldl_step(A, ld, n, k, r); });
}

// forward then backward substitution on the factor in f.H: f.rhs -> f.qdd
template <typename T, typename Rows>
IKG_HD inline void ctl_substitute(const CtlWs<T>& f, Rows& rows) {
#pragma unroll 1
  for (int k = 0; k < f.nq; ++k) rows([&](int r) { ctl_solve_fwd(f, k, r); });
#pragma unroll 1
  for (int k = f.nq - 1; k >= 0; --k) rows([&](int r) { ctl_solve_bwd(f, k, r); });
}

// the solve of one state whose workspace is loaded, up to w.qdd
template <typename T, typename Rows>
IKG_HD inline void control_solve_phases(const CtlWs<T>& w, const KCtl<T>& p, Rows& rows) {
  ldl_factor(w.M, w.ld, w.nq, rows);
  rows([&](int r) { ctl_pivots(w, r); });
  rows([&](int r) { ctl_forward(w, p, r); });
  rows([&](int r) { ctl_opspace(w, p, r); });
#pragma unroll 1
  for (int k = 0; k < 6; ++k) rows([&](int r) { ctl_opspace_step(w, k, r); });
  rows([&](int r) { ctl_lambda(w, p, r, rows.lam(r)); });
  rows([&](int r) { ctl_normal(w, p, r); });
  ldl_factor(w.H, w.ld, w.nq, rows);
  rows([&](int r) { ctl_check(w, r); });
  ctl_substitute(w, rows);
}

template <typename T>
inline void control_ws_load(const CtlWs<T>& w, const T* M, const T* nle, const T* J, const T* dJv, const T* e,
                            const T* ed) {
  const int nq = w.nq;
  for (int r = 0; r < nq; ++r) {
    for (int c = 0; c < nq; ++c) w.M[r * w.ld + c] = M[r * nq + c];
    w.Md[r] = M[r * nq + r];
    w.nle[r] = nle[r];
  }
  for (int k = 0; k < 12; ++k) {
    for (int r = 0; r < nq; ++r) w.J[k * w.ld + r] = J[k * nq + r];
    w.dJv[k] = dJv[k];
    w.e[k] = e[k];
    w.ed[k] = ed[k];
  }
}

// One state on the host: the phases in the kernel's order.  M [nq,nq], nle
// [nq], J [12,nq], dJv / e / ed [12] in; outputs may be null.
template <typename T>
inline void control_state(int nq, const KCtl<T>& p, const T* M, const T* nle, const T* J, const T* dJv, const T* e,
                          const T* ed, T* tau, T* qdd, T* xdd, T* Lambda, T* fc) {
  T buf[2 * kMaxNq * (kMaxNq + 1) + 24 * (kMaxNq + 1) + 6 * kMaxNq + 146];
  CtlWs<T> w;
  ctl_ws_bind(buf, nq, w);
  control_ws_load(w, M, nle, J, dJv, e, ed);
  HostRows<T> rows{nq > 12 ? nq : 12, Lambda};
  control_solve_phases(w, p, rows);
  for (int r = 0; r < nq; ++r) {
    const T t = ctl_tau(w, p, r);
    if (tau) tau[r] = t;
    if (qdd) qdd[r] = w.qdd[r];
  }
  for (int k = 0; k < 12; ++k) {
    if (xdd) xdd[k] = w.xdd[k];
    if (fc) fc[k] = w.fc[k];
  }
}

// ---------------------------------------------------------------- Bezier desired state (control.py:30-46)
// The reference's Bezier.__call__ / eval_horner, operation for operation:
//   u = (t - T_min) / (T_max - T_min);  u_op = 1 - u;  tmp = P_0 u_op
//   for i in 1 .. degree - 1:  tn *= u;  bc *= (degree - i + 1) / i;  tmp = (tmp + (tn bc) P_i) u_op
//   result = (tmp + (tn u) P_degree) mult
// and mult P_0 for a curve of two control points (the reference's size_ == 1
// branch).  The binomial factors bc_i do not depend on t: bezier_coeffs builds
// them once on the host with the reference's operations.  P is [n, dim]
// row-major, one column per joint; the caller keeps t in [t_min, t_max].
constexpr int kMaxBezier = 64;  // control points of a curve

template <typename T>
struct KBezier {
  const T* P;   // [n, dim]
  const T* bc;  // [n]; bc[0] = 1
  int n, dim;
  T t_min, t_max, mult;
};

inline void bezier_coeffs(int n, double* bc) {
  const int degree = n - 1;
  double b = 1.0;
  bc[0] = 1.0;
  for (int i = 1; i < n; ++i) {
    b *= (double)(degree - i + 1) / (double)i;
    bc[i] = b;
  }
}

template <typename T>
IKG_HD inline T bezier_clamp(const KBezier<T>& c, T t) {
  return t < c.t_min ? c.t_min : (t > c.t_max ? c.t_max : t);
}

// No contraction into fused multiply-adds: the init kernel, the step kernel,
// the evaluation kernel and the host all round every product as the reference's
// numpy does, so a desired state does not depend on which of them computed it
// (a rollout of 8 ticks equals 8 rollouts of 1 tick to the bit).
template <typename T>
IKG_HD inline T bezier_eval(const KBezier<T>& c, T t, int col) {
#pragma clang fp contract(off)
  if (c.n == 2) return c.mult * c.P[col];
  const T u = (t - c.t_min) / (c.t_max - c.t_min);
  const T uo = T(1) - u;
  T tn = T(1);
  T tmp = c.P[col] * uo;
  for (int i = 1; i < c.n - 1; ++i) {
    tn *= u;
    tmp = (tmp + (tn * c.bc[i]) * c.P[i * c.dim + col]) * uo;
  }
  return (tmp + (tn * u) * c.P[(c.n - 1) * c.dim + col]) * c.mult;
}

// ---------------------------------------------------------------- forward dynamics and one closed-loop tick
// qdd = M^-1 (tau - nle) with the L D L^T factor of M (ldl_step) and the
// substitution phases of the QP (ctl_solve_fwd / ctl_solve_bwd): fd_view
// presents the factor as their H, with a pivot flag of its own (the QP's flag
// zeroes the QP's answer, not the plant's).
template <typename T>
IKG_HD inline void fd_view(const CtlWs<T>& w, T* flag, CtlWs<T>& f) {
  f = w;
  f.H = w.M;
  f.fail = flag;
}

// a state's workspace of the closed-loop step: the solve's plus the flag above
IKG_HD inline int step_ws_len(int nq) { return ctl_ws_len(nq) + 2; }

// row r: the applied torque and the right-hand side tau - nle of the forward dynamics
template <typename T>
IKG_HD inline T step_rhs(const CtlWs<T>& w, const KCtl<T>& p, T* flag, int r) {
  T t = T(0);
  if (r < w.nq) {
    t = ctl_tau(w, p, r);
    w.rhs[r] = t - w.nle[r];
  }
  if (r == 0) *flag = T(0);
  return t;
}

// semi-implicit Euler (Bullet's scheme): v += dt qdd, then q += dt v
template <typename T>
IKG_HD inline void step_integrate(T dt, T qdd, T& q, T& v) {
  v += dt * qdd;
  q += dt * v;
}

// the forward-dynamics workspace on its own: M [nq*ld] (factored in place), rhs, qdd [nq], flag
IKG_HD inline int fd_ws_len(int nq) { return nq * (nq | 1) + 2 * nq + 2; }

template <typename T>
IKG_HD inline void fd_ws_bind(T* base, int nq, CtlWs<T>& f) {
  const int ld = nq | 1;
  f.nq = nq;
  f.ld = ld;
  f.M = f.H = base;
  f.rhs = base + nq * ld;
  f.qdd = f.rhs + nq;
  f.fail = f.qdd + nq;
  f.Md = f.Mr = f.Ms = f.J = f.Z = f.A = f.nle = f.e = f.ed = f.dJv = f.fc = f.xdd = nullptr;
}

// One state on the host: qdd = M^-1 (tau - nle), the forward-dynamics kernel's order
template <typename T>
inline void forward_dynamics_state(int nq, const T* M, const T* nle, const T* tau, T* qdd) {
  T buf[kMaxNq * (kMaxNq + 1) + 2 * kMaxNq + 2];
  CtlWs<T> f;
  fd_ws_bind(buf, nq, f);
  for (int r = 0; r < nq; ++r) {
    for (int c = 0; c < nq; ++c) f.M[r * f.ld + c] = M[r * nq + c];
    f.rhs[r] = tau[r] - nle[r];
  }
  *f.fail = T(0);
  HostRows<T> rows{nq, nullptr};
  ldl_factor(f.M, f.ld, nq, rows);
  ctl_substitute(f, rows);
  for (int r = 0; r < nq; ++r) qdd[r] = f.qdd[r];
}

// One closed-loop tick of one state on the host, the step kernel's order: the
// solve's phases, tau, the forward dynamics on the factor of M the solve left,
// the integrator.  q, v [nq] are advanced in place; tau [nq] out.
template <typename T>
inline void control_step_state(int nq, const KCtl<T>& p, const T* M, const T* nle, const T* J, const T* dJv,
                               const T* e, const T* ed, T dt, T* q, T* v, T* tau) {
  T buf[2 * kMaxNq * (kMaxNq + 1) + 24 * (kMaxNq + 1) + 6 * kMaxNq + 148];
  CtlWs<T> w, f;
  ctl_ws_bind(buf, nq, w);
  T* flag = buf + ctl_ws_len(nq);
  control_ws_load(w, M, nle, J, dJv, e, ed);
  HostRows<T> rows{nq > 12 ? nq : 12, nullptr};
  control_solve_phases(w, p, rows);
  for (int r = 0; r < nq; ++r) tau[r] = step_rhs(w, p, flag, r);
  fd_view(w, flag, f);
  ctl_substitute(f, rows);
  for (int r = 0; r < nq; ++r) step_integrate(dt, f.qdd[r], q[r], v[r]);
}

// ---------------------------------------------------------------- inverse dynamics along curves
// ikg_trajectory_dynamics_batch: recursive Newton-Euler with the joint
// acceleration included, tau = rnea(q, qd, qdd), beside g = rnea(q, 0, 0), at
// the samples of a curve, and the actuator-limit ratios folded per curve.  M is
// never formed.
//
// dyn_forward with the joint acceleration: a_i = a_p + S_i qdd_i + (v_i x S_i) qd_i.
// A function of its own beside dyn_forward: the existing kernels keep theirs as
// it is (sharing the forward pass moved their last bits, ikg_dynamics.hip).
template <typename T>
IKG_HD inline void dyn_forward_acc(const DynBody<T>& par, const T* jR, const T* jt, int axis, T s, T c, T qd, T qdd,
                                   DynBody<T>& b, T* S) {
  T P[9], d[3], ax[3];
  matmul3(par.R, jR, P);
  matvec3(par.R, jt, d);
  const T e0 = T(axis == 0), e1 = T(axis == 1), e2 = T(axis == 2);
  const T omc = T(1) - c;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const T r0 = P[3 * r], r1 = P[3 * r + 1], r2 = P[3 * r + 2];
    const T u = e0 * r0 + e1 * r1 + e2 * r2;
    ax[r] = u;
    b.R[3 * r + 0] = c * r0 + s * (e2 * r1 - e1 * r2) + omc * u * e0;
    b.R[3 * r + 1] = c * r1 + s * (e0 * r2 - e2 * r0) + omc * u * e1;
    b.R[3 * r + 2] = c * r2 + s * (e1 * r0 - e0 * r1) + omc * u * e2;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) b.o[i] = par.o[i] + d[i];
  dcross(b.o, ax, S);
#pragma unroll
  for (int i = 0; i < 3; ++i) S[3 + i] = ax[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) b.v[i] = par.v[i] + S[i] * qd;
  T t1[3], t2[3], t3[3];
  dcross(b.v + 3, S, t1);
  dcross(b.v, S + 3, t2);
  dcross(b.v + 3, S + 3, t3);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    b.a[i] = par.a[i] + S[i] * qdd + (t1[i] + t2[i]) * qd;
    b.a[3 + i] = par.a[3 + i] + S[3 + i] * qdd + t3[i] * qd;
  }
}

// One state on the host in the trajectory-dynamics kernel's order: forward pass
// with accelerations, both forces per body, subtree sums over j ascending.
// tau [nq] = rnea(q, v, a), g [nq] = rnea(q, 0, 0).
template <typename T>
inline void inverse_dynamics_state(const KModel<T>& m, const KInertia<T>& in, const T* q, const T* v, const T* a,
                                   T* tau, T* g) {
  const int nq = m.nq;
  DynBody<T> body[kMaxNq], uni;
  T S[kMaxNq][6], f[kMaxNq][6], f0[kMaxNq][6];
  dyn_universe(in.grav, in.ref, uni);
  const T zero[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  for (int i = 0; i < nq; ++i) {
    T s, c;
    cw_sincos(q[i], &s, &c);
    const DynBody<T>& par = m.jparent[i] >= 0 ? body[m.jparent[i]] : uni;
    dyn_forward_acc(par, m.jR[i], m.jt[i], m.jaxis[i], s, c, v[i], a[i], body[i], S[i]);
    DynInertia<T> W;
    dyn_inertia_world(in.mass[i], in.h[i], in.Io[i], body[i].R, body[i].o, W);
    dyn_force(W, body[i].v, body[i].a, f[i]);
    dyn_force(W, zero, uni.a, f0[i]);
  }
  for (int i = 0; i < nq; ++i) {
    T fc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, gc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    for (int j = 0; j < nq; ++j)
      if ((in.anc[j] >> i) & 1)
        for (int k = 0; k < 6; ++k) {
          fc[k] += f[j][k];
          gc[k] += f0[j][k];
        }
    tau[i] = ddot6(S[i], fc);
    g[i] = ddot6(S[i], gc);
  }
}

// Control point i, column col, of a curve's derivative (Bezier.derivative):
// degree (P[i+1] - P[i]), the difference and the product each rounded
template <typename T>
IKG_HD inline T bezier_derivative_point(const T* P, int n_points, int dim, int i, int col) {
#pragma clang fp contract(off)
  const T d = P[(i + 1) * dim + col] - P[i * dim + col];
  return T(n_points - 1) * d;
}

constexpr double kNoLimit = 1e30;   // IKG_NO_LIMIT
constexpr int kTrajDynMinPoints = 5;  // below degree 4 the acceleration curve has two control points

// A maximum with where it was found; among exact ties the lowest sample, then the lowest joint.
// sample < 0: nothing folded yet.
struct DynPeak {
  double val;
  int32_t sample, joint;
};

IKG_HD inline void peak_init(DynPeak& p) {
  p.val = -1.0;
  p.sample = p.joint = -1;
}

// order-independent: the larger value, then the lower (sample, joint)
IKG_HD inline void peak_merge(DynPeak& a, const DynPeak& b) {
  if (b.sample < 0) return;
  const bool first = b.sample < a.sample || (b.sample == a.sample && b.joint < a.joint);
  if (a.sample < 0 || b.val > a.val || (b.val == a.val && first)) a = b;
}

// A run of samples of one curve, folded: what a wave leaves in the scratch
struct TrajDynPartial {
  DynPeak speed, torque_use, static_use, torque_scale;
  int32_t n_static, pad;
};

IKG_HD inline void dynpartial_init(TrajDynPartial& p) {
  peak_init(p.speed);
  peak_init(p.torque_use);
  peak_init(p.static_use);
  peak_init(p.torque_scale);
  p.n_static = p.pad = 0;
}

IKG_HD inline void dynpartial_merge(TrajDynPartial& a, const TrajDynPartial& b) {
  peak_merge(a.speed, b.speed);
  peak_merge(a.torque_use, b.torque_use);
  peak_merge(a.static_use, b.static_use);
  peak_merge(a.torque_scale, b.torque_scale);
  a.n_static += b.n_static;
}

// Entry (sample k, joint j) with velocity v, torques tau and g under the limits
// vlim, E (kNoLimit: the joint contributes 0):
//   speed |v| / vlim, torque use |tau| / E, static use |g| / E;
//   |g| >= E: no duration helps, counted in n_static and left out of torque_scale;
//   else with d = tau - g (scales as 1 / s^2 under t -> s t): the least s with
//   |g + d / s^2| <= E is sqrt(|d| / (E - sign(d) g)), 0 where d = 0.
IKG_HD inline void dynpartial_add(TrajDynPartial& p, int k, int j, double v, double tau, double g, double vlim,
                                  double E) {
  const bool vfree = vlim >= kNoLimit, efree = E >= kNoLimit;
  const DynPeak sp{vfree ? 0.0 : fabs(v) / vlim, k, j};
  const DynPeak tu{efree ? 0.0 : fabs(tau) / E, k, j};
  const DynPeak su{efree ? 0.0 : fabs(g) / E, k, j};
  peak_merge(p.speed, sp);
  peak_merge(p.torque_use, tu);
  peak_merge(p.static_use, su);
  if (!efree && fabs(g) >= E) {
    p.n_static += 1;
    return;
  }
  const double d = tau - g;
  double s = 0.0;
  if (!efree && d != 0.0) s = sqrt(fabs(d) / (d > 0.0 ? E - g : E + g));
  const DynPeak ts{s, k, j};
  peak_merge(p.torque_scale, ts);
}

// Samples per wave where the caller leaves it open: runs of whole lane groups
// (spg = 64 / G samples side by side) short enough for about kTrajDynWaves
// waves, at most S.
constexpr int64_t kTrajDynWaves = 8192;
IKG_HD inline int trajdyn_samples_per_wave(int64_t B, int S, int forced, int spg) {
  if (forced >= 1) return forced < S ? forced : S;
  const int64_t want = (kTrajDynWaves + B - 1) / B;  // runs per curve
  int64_t spw = (S + want - 1) / want;
  spw = (spw + spg - 1) / spg * spg;
  return (int)(spw < 1 ? 1 : (spw > S ? S : spw));
}

struct TrajDynArgs {
  const double* points;  // [B, n_points, nq]
  int n_points;
  double t_min, t_max, mult, mult_v, mult_a;  // mult_v = mult (1 / T), mult_a = mult_v (1 / T)
  int S, spw, chunks;
  double *tau, *g;       // [B, S, nq], optional
  TrajDynPartial* part;  // [B * chunks]
  double bc[3][kMaxBezier];  // bezier_coeffs of the q, v and a curves
  double vlim[kMaxNq], elim[kMaxNq];
};

// the curves' multipliers and binomial factors as Bezier.derivative forms them
inline void trajdyn_curve_setup(TrajDynArgs& a) {
  const double inv = 1.0 / (a.t_max - a.t_min);
  a.mult_v = a.mult * inv;
  a.mult_a = a.mult_v * inv;
  std::memset(a.bc, 0, sizeof(a.bc));
  for (int d = 0; d < 3; ++d) bezier_coeffs(a.n_points - d, a.bc[d]);
}

struct TrajDynFoldOut {
  double* speed_scale;
  int32_t* arg_speed;  // [B,2] (sample, joint)
  double* torque_use;
  int32_t* arg_torque_use;
  double* static_use;
  int32_t* arg_static;
  int32_t* n_static;
  double* torque_scale;
  int32_t* arg_torque_scale;
};

IKG_HD inline void peak_store(double* val, int32_t* arg, int64_t b, const DynPeak& p) {
  if (val) val[b] = p.sample < 0 ? 0.0 : p.val;
  if (arg) {
    arg[2 * b] = p.sample;
    arg[2 * b + 1] = p.joint;
  }
}

IKG_HD inline void dynfold_store(const TrajDynFoldOut& o, int64_t b, const TrajDynPartial& p) {
  peak_store(o.speed_scale, o.arg_speed, b, p.speed);
  peak_store(o.torque_use, o.arg_torque_use, b, p.torque_use);
  peak_store(o.static_use, o.arg_static, b, p.static_use);
  peak_store(o.torque_scale, o.arg_torque_scale, b, p.torque_scale);
  if (o.n_static) o.n_static[b] = p.n_static;
}

hipError_t launch_trajdyn(const KModel<double>* dm, const KInertia<double>* di, int nq, const TrajDynArgs& a, int64_t B,
                          const TrajDynFoldOut& o, hipStream_t s);

}  // namespace ikg
