// Host emulator of the pair kernel (debug/test tool, NOT a product path and
// never called by libikgrasp.so): runs the exact stage functions of
// ikg_device.hpp for both arm lanes of a problem on the CPU, in the order the
// kernel's lanes execute them, so kernel numerics can be inspected without a
// GPU.  Built as libikgrasp_emu.so.  Further down: the collision, dynamics,
// controller and closed-loop rollout arithmetic on the same terms.
// The library has no header: tests/emu.py's PROTOTYPES is its one declaration,
// used by every test and tool, and tests/test_emu_binding.py compares that table
// with the definitions in this file.  A new `extern "C"` export needs a row there.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

// ikg_emu_force_small_angle's switch, read by log6_iter<double, COLD> through this macro (the
// product units compile it as false, ikg_device.hpp)
thread_local bool ikg_emu_small_angle = false;
#define IKG_EMU_SMALL_ANGLE() (::ikg_emu_small_angle)
#include "ikg_collision.hpp"
#include "ikg_device.hpp"
#include "ikg_dynamics.hpp"
#include "ikg_fit.hpp"
#include "ikg_model_build.hpp"
#include "ikg_planner.hpp"
#include "ikg_trajcheck.hpp"
#include "ikgrasp.h"

namespace {

// updates that took the LQ form (pinv_step_*), since the last ikg_emu_lq_count(1)
thread_local long long lq_count = 0;
thread_local long long big_count = 0;  // lane-updates whose step leaves the short trig series (chest-frame path)
thread_local long long jacobi_count = 0;  // arm solves of the LQ form that fell back to the Jacobi sweeps
thread_local long long svd_count = 0;  // of those, with an arm that pins the chest (bb = 0: rank-deficient M_a)
// updates whose two arm lanes computed different chest steps (must stay 0:
// each lane carries the shared chest joint); ikg_emu_solve returns -3 then
thread_local long long chest_mismatch = 0;
// ikg_emu_force_general(1): the general pose error for z-aligned targets too (the loop a wave
// runs when it also holds another target); tests/test_zaligned.py compares the two
thread_local bool force_general = false;

// collide_wave's stages run serially (same functions, same order per lane).
template <typename T>
bool emu_collide(const ikg::KModel<T>& m, const ikg::KCollision<T>& c, const T* q, const T* tgt) {
  using namespace ikg;
  T L[kMaxNq][12], F[kMaxNq][12], P[kMaxGeoms][12];
  for (int j = 0; j < m.nq; ++j) {
    T s, co;
    Prec<T>::sincos_(q[j], &s, &co);
    joint_local(&m, j, s, co, L[j]);
  }
  for (int j = 0; j < m.nq; ++j) joint_world(m.jparent, j, L, F[j]);
  for (int g = 0; g < c.n_geoms; ++g) geom_world(&c, g, F, tgt, P[g]);
  for (int k = 0; k < c.n_pairs; ++k)
    if (pair_hit(&c, k, P)) return true;
  return false;
}

template <typename T, class SP>
void emu_one(const ikg::KModel<T>& m, const ikg::KParams<T>& prm, bool damped, const T* tg, const T* qrow,
             T* qo, uint8_t* conv_out, int32_t* iters_out, T* err_out, T* trace, int trace_len,
             const ikg::KCollision<T>* col, bool med = false) {
  using namespace ikg;
  T RT[2][9], tT[2][3], qc[2], qa[2][kArmDof], sn[2][7], cs[2][7];
  for (int arm = 0; arm < 2; ++arm) {
    const bool right = arm != 0;
    T HR[9], Ht[3], d[3];
    for (int i = 0; i < 9; ++i) HR[i] = right ? m.hook_R[1][i] : m.hook_R[0][i];
    for (int i = 0; i < 3; ++i) Ht[i] = right ? m.hook_t[1][i] : m.hook_t[0][i];
    matmul3(tg, HR, RT[arm]);
    matvec3(tg, Ht, d);
    for (int i = 0; i < 3; ++i) tT[arm][i] = tg[9 + i] + d[i];
    qc[arm] = qrow[m.root_q];
    for (int k = 0; k < kArmDof; ++k) qa[arm][k] = qrow[m.arm_q[arm][k]];
  }
  // the kernel's choice (pair_batch_body) for a wave that holds this problem alone
  const bool zt = !force_general && z_aligned(RT[0]) && z_aligned(RT[1]);
  int it = 0;
  bool conv = false;
  T nrm[2];
  ThetaTrack<T> tk[2] = {};
  // the kernel's frame-1 path (kFrame1 models, lambda = 0) or the chest-frame one
  const bool f1 = kFrame1<SP> && !damped;
  for (int arm = 0; arm < 2; ++arm) {
    if (f1)
      trig_exact_f1(&m, arm, qc[arm], qa[arm], sn[arm], cs[arm]);
    else
      trig_exact(qc[arm], qa[arm], sn[arm], cs[arm]);
  }
  for (;;) {
    ArmState<T> st[2];
    ArmStateF1<T> s1[2];
    const bool resync = (it % Trig<T>::kResync) == 0;
    ThetaTrack<T>* tkp[2] = {is_f64<T> ? &tk[0] : nullptr, is_f64<T> ? &tk[1] : nullptr};
    for (int arm = 0; arm < 2; ++arm) {
      if constexpr (kFrame1<SP>) {
        if (f1) {
          // fp64: the pose error as the record-free pair loop instantiates it (COLD: log6_iter's
          // rare branch, which ikg_emu_force_small_angle holds taken).  The checkpoint, resume and
          // quad kernels instantiate COLD = false: the same values (a resync forces the exact angle
          // either way, and a lane outside both bands keeps the forms the selects pick for it), but
          // log6_iter's non-COLD fp64 text is reached only through ikg_emu_se3 (fn 4, 5) now.
          constexpr bool CD = is_f64<T>;
          nrm[arm] = (zt ? arm_fk_error_f1<T, SP, CD, true> : arm_fk_error_f1<T, SP, CD, false>)(
              &m, arm, sn[arm], cs[arm], RT[arm], tT[arm], s1[arm], tkp[arm], resync);
          continue;
        }
      }
      nrm[arm] = arm_fk_error<T, SP>(&m, arm, sn[arm], cs[arm], RT[arm], tT[arm], st[arm], nullptr, tkp[arm], resync);
    }
    if (trace && it < trace_len) {
      trace[2 * it] = std::sqrt(nrm[0]);
      trace[2 * it + 1] = std::sqrt(nrm[1]);
    }
    if (it >= prm.max_iters) break;
    if (nrm[0] < prm.eps2 && nrm[1] < prm.eps2) {
      if (!col) {
        conv = true;
        break;
      }
      T qn[kMaxNq];  // the current iterate in q order (passive joints clamped after update 1)
      for (int j = 0; j < m.nq; ++j) qn[j] = qrow[j];
      for (int i = 0; i < m.n_passive; ++i) {
        const int j = m.passive_q[i];
        qn[j] = it > 0 ? clampq(qrow[j], m.lo[j], m.hi[j]) : qrow[j];
      }
      qn[m.root_q] = qc[0];
      for (int arm = 0; arm < 2; ++arm)
        for (int k = 0; k < kArmDof; ++k) qn[m.arm_q[arm][k]] = qa[arm][k];
      if (!emu_collide(m, *col, qn, tg)) {
        conv = true;
        break;
      }
    }
    T A[2][6][8], u[2][6], v[2][6], al[2], be[2], dqa[2][6], sa[2], q_old[2][7];
    bool bad[2] = {false, false};
    for (int arm = 0; arm < 2; ++arm) {
      q_old[arm][0] = qc[arm];
      for (int k = 0; k < kArmDof; ++k) q_old[arm][k + 1] = qa[arm][k];
      if constexpr (kFrame1<SP>) {
        if (f1) {
          arm_solve_f1<T, SP>(&m, arm, s1[arm], sn[arm], cs[arm], u[arm], v[arm], al[arm], be[arm]);
          bad[arm] = beyond(be[arm], m.sing_beta);
          continue;
        }
      }
      if (damped) {
        arm_system(st[arm], A[arm]);
        arm_solve_damped(A[arm], prm.lambda, u[arm], v[arm], al[arm], be[arm]);
      } else {
        arm_solve<T, SP>(st[arm], u[arm], v[arm], al[arm], be[arm], &bad[arm], m.sing_tau);
        bad[arm] = bad[arm] || beyond(be[arm], m.sing_beta);
      }
    }
    for (int arm = 0; arm < 2; ++arm) {
      if (damped) {
        T t_o;
        damped_couple(al[arm], be[arm], al[1 - arm], be[1 - arm], sa[arm], t_o);
        arm_dq_damped(A[arm], u[arm], v[arm], t_o, dqa[arm]);
      } else {
        sa[arm] = chest_step(al[arm] + al[1 - arm], be[arm] + be[1 - arm]);
        arm_dq(u[arm], v[arm], sa[arm], dqa[arm]);
      }
    }
    if (!damped && (bad[0] || bad[1])) {  // pinv_step_f1 / pinv_step_cf: the per-arm pinv form
      T z[2][7], pv[2][7];
      for (int arm = 0; arm < 2; ++arm) {
        if (f1) {
          if constexpr (kFrame1<SP>) arm_system_f1<T, SP>(&m, arm, s1[arm], sn[arm], cs[arm], A[arm]);
        } else {
          arm_system(st[arm], A[arm]);
        }
        if (!arm_minnorm(A[arm], z[arm], pv[arm])) ++jacobi_count;
      }
      for (int arm = 0; arm < 2; ++arm) {
        T f;
        minnorm_combine(z[arm][0], pv[arm][0], z[1 - arm][0], pv[1 - arm][0], sa[arm], f);
        for (int k = 0; k < 6; ++k) dqa[arm][k] = z[arm][1 + k] + f * pv[arm][1 + k];
      }
      if (sa[0] != sa[1]) ++chest_mismatch;  // both lanes must carry the same chest step
      ++lq_count;
      if (pv[0][0] < T(Prec<T>::kRcond) || pv[1][0] < T(Prec<T>::kRcond)) ++svd_count;  // an arm pins s
    }
    ++it;
    for (int arm = 0; arm < 2; ++arm) {
      const T s = sa[arm];
      const T* dq = dqa[arm];
      ArmLimits<T> lim;
      load_limits(&m, arm, lim);
      arm_update(&m, arm, prm.dt, s, dq, qc[arm], qa[arm], &lim);
      if (f1)
        (med ? trig_advance_f1<T, true> : trig_advance_f1<T, false>)(&m, arm, qc[arm], qa[arm], q_old[arm],
                                                                     (it % Trig<T>::kResync) == 0, sn[arm], cs[arm]);
      else {
        bool big = false;  // the exact sincos outside resyncs (diagnostic count)
        big |= fabs(qc[arm] - q_old[arm][0]) > T(Trig<T>::kIncMax);
        for (int k = 0; k < kArmDof; ++k) big |= fabs(qa[arm][k] - q_old[arm][k + 1]) > T(Trig<T>::kIncMax);
        if (big) ++big_count;
        trig_advance<T, IKG_GENERIC_MED>(qc[arm], qa[arm], q_old[arm], (it % Trig<T>::kResync) == 0, sn[arm], cs[arm]);
      }
    }
  }
  for (int j = 0; j < m.nq; ++j) qo[j] = qrow[j];
  for (int i = 0; i < m.n_passive; ++i) {
    const int j = m.passive_q[i];
    qo[j] = it > 0 ? clampq(qrow[j], m.lo[j], m.hi[j]) : qrow[j];
  }
  qo[m.root_q] = qc[0];
  for (int arm = 0; arm < 2; ++arm)
    for (int k = 0; k < kArmDof; ++k) qo[m.arm_q[arm][k]] = qa[arm][k];
  *conv_out = conv;
  *iters_out = it;
  err_out[0] = std::sqrt(nrm[0]);
  err_out[1] = std::sqrt(nrm[1]);
}

template <typename T>
void emu(const ikg_model_desc* d, const void* targets, const void* q0, int64_t stride, int64_t B,
         const ikg_params* p, void* q_out, uint8_t* conv, int32_t* iters, void* err, void* trace, int trace_len,
         const ikg_collision_desc* cd) {
  ikg::KModel<T> m;
  ikg::build_kmodel<T>(*d, m);
  static thread_local ikg::KCollision<T> kc;
  const ikg::KCollision<T>* col = nullptr;
  if (cd && p->check_collision) {
    ikg::build_kcollision<T>(*cd, kc);
    col = &kc;
  }
  const ikg::KParams<T> prm = ikg::make_kparams<T>(p);
  const int spec = p->variant == 99 ? 0 : ikg::choose_spec(m);  // variant 99: force generic
  for (int64_t i = 0; i < B; ++i) {
    const T* tg = (const T*)targets + 12 * i;
    const T* qr = (const T*)q0 + stride * i;
    T* tr = trace ? (T*)trace + (int64_t)2 * trace_len * i : nullptr;
    if (spec == 1)
      // the kernels' medium-range trig series for per-problem seeds, and for
      // every fp32 solve (ikg_kernels.hip launch_pair_batch_t)
      emu_one<T, ikg::SpecNextage>(m, prm, p->lambda > 0, tg, qr, (T*)q_out + d->nq * i, conv + i, iters + i,
                                   (T*)err + 2 * i, tr, trace_len, col, stride != 0 || sizeof(T) == 4);
    else if (spec == 2 && !(p->lambda > 0))
      emu_one<T, ikg::SpecGenericWrist>(m, prm, false, tg, qr, (T*)q_out + d->nq * i, conv + i, iters + i,
                                        (T*)err + 2 * i, tr, trace_len, col);
    else
      emu_one<T, ikg::SpecGeneric>(m, prm, p->lambda > 0, tg, qr, (T*)q_out + d->nq * i, conv + i, iters + i,
                                   (T*)err + 2 * i, tr, trace_len, col);
  }
}

}  // namespace

extern "C" long long ikg_emu_big_count(int reset) {
  const long long v = big_count;
  if (reset) big_count = 0;
  return v;
}
extern "C" long long ikg_emu_lq_count(int reset) {
  const long long v = lq_count;
  if (reset) lq_count = 0;
  return v;
}
extern "C" long long ikg_emu_jacobi_count(int reset) {
  const long long v = jacobi_count;
  if (reset) jacobi_count = 0;
  return v;
}
extern "C" long long ikg_emu_svd_count(int reset) {
  const long long v = svd_count;
  if (reset) svd_count = 0;
  return v;
}

// cd may be NULL; it is used when p->check_collision is set.
// Returns 0, or -3 when the two lanes of a problem ever carried different
// chest steps (a kernel invariant; the outputs are then not the kernel's).
extern "C" int ikg_emu_solve(const ikg_model_desc* d, int dtype, const void* targets, const void* q0,
                             int64_t q0_stride, int64_t B, const ikg_params* p, void* q_out, uint8_t* conv,
                             int32_t* iters, void* err, void* trace, int trace_len, const ikg_collision_desc* cd) {
  chest_mismatch = 0;
  if (dtype == IKG_F64)
    emu<double>(d, targets, q0, q0_stride, B, p, q_out, conv, iters, err, trace, trace_len, cd);
  else
    emu<float>(d, targets, q0, q0_stride, B, p, q_out, conv, iters, err, trace, trace_len, cd);
  return chest_mismatch ? -3 : 0;
}

// The general pose-error loop for every target (on != 0), or the kernel's choice (0).
extern "C" void ikg_emu_force_general(int on) { force_general = on != 0; }

// log6_iter's rare branch (fp64 pair loop: the small-angle forms and the near-pi axis behind
// their selects) on every update (on != 0), as a lane runs it whose wave-mates hold the branch
// taken, or only where this problem's own angle asks for it (0); tests/test_log6_rare_path.py
extern "C" void ikg_emu_force_small_angle(int on) { ikg_emu_small_angle = on != 0; }

// The end of one update of the fp64 pair loop (integrate + clamp, trig advance) for n cases of one
// arm each: staged = 0 runs arm_update (the `lim` path), staged != 0 the stage-by-stage form the
// record-free kernel runs (arm_update_staged), either followed by trig_advance_f1<double, false,
// true>; tests/test_seam_stage_order.py compares their bits.  in [n][22]: s, dq[6], qc, qa[6],
// sn[7], resync flag; cs [n][7]; out [n][21]: qc, qa[6], sn[7], cs[7].
extern "C" int ikg_emu_seam(const ikg_model_desc* d, int staged, int64_t n, const int32_t* arm, double dt,
                            const double* in, const double* cs_in, double* out) {
  using namespace ikg;
  static thread_local KModel<double> m;
  build_kmodel<double>(*d, m);
  for (int64_t i = 0; i < n; ++i) {
    const double* x = in + 22 * i;
    const double s = x[0];
    double dq[6], qc = x[7], qa[kArmDof], q_old[7], sn[7], cs[7];
    for (int k = 0; k < 6; ++k) dq[k] = x[1 + k];
    for (int k = 0; k < kArmDof; ++k) qa[k] = x[8 + k];
    for (int j = 0; j < 7; ++j) sn[j] = x[14 + j], cs[j] = cs_in[7 * i + j];
    const bool resync = x[21] != 0.0;
    q_old[0] = qc;
    for (int k = 0; k < kArmDof; ++k) q_old[k + 1] = qa[k];
    ArmLimits<double> lim;
    load_limits(&m, arm[i], lim);
    if (staged)
      arm_update_staged<double>(&m, dt, s, dq, qc, qa, lim);
    else
      arm_update(&m, arm[i], dt, s, dq, qc, qa, &lim);
    trig_advance_f1<double, false, true>(&m, arm[i], qc, qa, q_old, resync, sn, cs);
    double* o = out + 21 * i;
    o[0] = qc;
    for (int k = 0; k < kArmDof; ++k) o[1 + k] = qa[k];
    for (int j = 0; j < 7; ++j) o[7 + j] = sn[j], o[14 + j] = cs[j];
  }
  return 0;
}

// The kernel's z-aligned test (z_aligned on hook_target's rotation) of n targets
// [n][12]: out[2 i + arm] = 1 where arm's hook target of target i passes.
template <typename T>
void emu_z_aligned(const ikg_model_desc* d, const void* targets, int64_t n, uint8_t* out) {
  static thread_local ikg::KModel<T> m;
  ikg::build_kmodel<T>(*d, m);
  for (int64_t i = 0; i < n; ++i)
    for (int arm = 0; arm < 2; ++arm) {
      T RT[9], tT[3];
      ikg::hook_target(&m, arm, (const T*)targets + 12 * i, RT, tT);
      out[2 * i + arm] = ikg::z_aligned(RT) ? 1 : 0;
    }
}
extern "C" int ikg_emu_z_aligned(const ikg_model_desc* d, int dtype, const void* targets, int64_t n, uint8_t* out) {
  if (dtype == IKG_F64)
    emu_z_aligned<double>(d, targets, n, out);
  else
    emu_z_aligned<float>(d, targets, n, out);
  return 0;
}

// Which tables and specialisation a model gets (tests/test_robot_family.py):
// build_kmodel<double> and choose_spec, read-only.  out = spec, wrist,
// hand_axis, rot_mask, zmask, pattern, n_passive, nq.
extern "C" int ikg_emu_model_info(const ikg_model_desc* d, int32_t out[8]) {
  static thread_local ikg::KModel<double> m;
  ikg::build_kmodel<double>(*d, m);
  out[0] = ikg::choose_spec(m);
  out[1] = m.wrist;
  out[2] = m.hand_axis;
  out[3] = m.rot_mask;
  out[4] = m.zmask;
  out[5] = m.pattern;
  out[6] = m.n_passive;
  out[7] = m.nq;
  return 0;
}

template <typename T>
void emu_col(const ikg_model_desc* d, const ikg_collision_desc* cd, const void* q, const void* targets, int64_t B,
             uint8_t* out) {
  ikg::KModel<T> m;
  ikg::build_kmodel<T>(*d, m);
  static thread_local ikg::KCollision<T> kc;
  ikg::build_kcollision<T>(*cd, kc);
  for (int64_t i = 0; i < B; ++i)
    out[i] = emu_collide(m, kc, (const T*)q + d->nq * i, (const T*)targets + 12 * i) ? 1 : 0;
}

// Collision query through the device stage functions (ikg_collision_batch on the CPU).
extern "C" int ikg_emu_collision(const ikg_model_desc* d, const ikg_collision_desc* cd, int dtype, const void* q,
                                 const void* targets, int64_t B, uint8_t* out) {
  if (dtype == IKG_F64)
    emu_col<double>(d, cd, q, targets, B, out);
  else
    emu_col<float>(d, cd, q, targets, B, out);
  return 0;
}

// Inscribed-ball certificate of scene pair `pair` at configuration qc (joint
// order = q order) with the cube at `target` (ball_cert, the records scan's
// certificate), then whether it proves the pair intersecting at each of the B
// configurations q (ball_covers).  tests/test_collision.py.
template <typename T>
void emu_ball(const ikg_model_desc* d, const ikg_collision_desc* cd, int pair, const void* qc, const void* target,
              const void* q, int64_t B, double* r_out, uint8_t* covered) {
  ikg::KModel<T> m;
  ikg::build_kmodel<T>(*d, m);
  static thread_local ikg::KCollision<T> kc;
  ikg::build_kcollision<T>(*cd, kc);
  int32_t sl[ikg::kMaxNq];
  for (int k = 0; k < ikg::kMaxNq; ++k) sl[k] = k;
  static thread_local ikg::BallCert<T> bc;
  ikg::ball_cert(&m, &kc, pair, (const T*)qc, sl, (const T*)target, bc);
  *r_out = (double)bc.r;
  for (int64_t i = 0; i < B; ++i) covered[i] = ikg::ball_covers(bc, (const T*)q + d->nq * i) ? 1 : 0;
}

extern "C" int ikg_emu_ball_cert(const ikg_model_desc* d, const ikg_collision_desc* cd, int dtype, int pair,
                                 const void* qc, const void* target, const void* q, int64_t B, double* r_out,
                                 uint8_t* covered) {
  if (pair < 0 || pair >= cd->n_pairs) return -1;
  if (dtype == IKG_F64)
    emu_ball<double>(d, cd, pair, qc, target, q, B, r_out, covered);
  else
    emu_ball<float>(d, cd, pair, qc, target, q, B, r_out, covered);
  return 0;
}

// EPA depth certificate of one shape pair (tests/test_collision_epa.py):
// kinds/placements/dims per ikg_collision_desc conventions; returns
// pair_collides' verdict in *r and the certified depth bound in *depth (0 when
// no certificate).
extern "C" int ikg_emu_epa(int kindA, const double* RA, const double* tA, const double* dA, int kindB,
                           const double* RB, const double* tB, const double* dB, int* r, double* depth) {
  using namespace ikg;
  const Shape<double> A{RA, tA, dA, kindA}, B{RB, tB, dB, kindB};
  double cert[12];
  *r = pair_collides(A, B, cert);
  *depth = 0.0;
  if (*r != 2) return 0;
  double pts[4][3];
  for (int k = 0; k < 4; ++k) mink_support(A, B, cert + 3 * k, pts[k]);
  if (!tetra_encloses_origin(pts[0], pts[1], pts[2], pts[3])) return 0;
  EpaScratch s;
  *depth = epa_depth_lb(A, B, pts, s);
  return 0;
}

// Narrow phase of n shape pairs (tests/test_primitives.py): kinds [n],
// placements [n][12] = R (row-major) then t, dims [n][3], as in
// ikg_collision_desc.  The placements and dimensions are rounded to the
// dtype as build_kcollision rounds the scene tables; hit = pair_collides<T>,
// dist = pair_distance<T>, dist_query = pair_distance<double> on the rounded
// values (what ikg_distance_kernel evaluates whatever its I/O type).
template <typename T>
void emu_pairs(int64_t n, const int32_t* kindA, const double* PA, const double* dA, const int32_t* kindB,
               const double* PB, const double* dB, uint8_t* hit, double* dist, double* dist_query) {
  using namespace ikg;
  for (int64_t i = 0; i < n; ++i) {
    T Pa[12], Pb[12], da[3], db[3];
    double Pa2[12], Pb2[12], da2[3], db2[3];
    for (int k = 0; k < 12; ++k) {
      Pa[k] = (T)PA[12 * i + k];
      Pb[k] = (T)PB[12 * i + k];
      Pa2[k] = (double)Pa[k];
      Pb2[k] = (double)Pb[k];
    }
    for (int k = 0; k < 3; ++k) {
      da[k] = (T)dA[3 * i + k];
      db[k] = (T)dB[3 * i + k];
      da2[k] = (double)da[k];
      db2[k] = (double)db[k];
    }
    const Shape<T> A{Pa, Pa + 9, da, kindA[i]}, B{Pb, Pb + 9, db, kindB[i]};
    hit[i] = pair_collides(A, B) != 0 ? 1 : 0;
    dist[i] = (double)pair_distance(A, B);
    const Shape<double> A2{Pa2, Pa2 + 9, da2, kindA[i]}, B2{Pb2, Pb2 + 9, db2, kindB[i]};
    dist_query[i] = pair_distance(A2, B2);
  }
}

extern "C" int ikg_emu_pairs(int dtype, int64_t n, const int32_t* kindA, const double* PA, const double* dA,
                             const int32_t* kindB, const double* PB, const double* dB, uint8_t* hit, double* dist,
                             double* dist_query) {
  if (dtype == IKG_F64)
    emu_pairs<double>(n, kindA, PA, dA, kindB, PB, dB, hit, dist, dist_query);
  else
    emu_pairs<float>(n, kindA, PA, dA, kindB, PB, dB, hit, dist, dist_query);
  return 0;
}

// The loop's math helpers over arrays (tests/test_host_emu.py accuracy checks):
// fn 0: cw_sincos (fp64), 1: cw_sincos (fp32), 2: the packed pair's sincos
// (both halves), 3: atan2_upper (fp32), 4: atan2_upper (packed pair).
// fn 5: Trig<double>::step, fn 6: the angle-addition form it replaced
// (step_addition): from the exact (sin, cos) of the angle y, Trig<double>::kResync
// consecutive steps of x with no resync (tests/test_trig_step.py).
// out holds 2 values per input (sin, cos) for fn 0-2, 1 for fn 3-4, 4 for fn
// 5-6 (the starting pair, then the pair after the steps).
extern "C" int ikg_emu_math(int fn, int64_t n, const double* x, const double* y, double* out) {
  using namespace ikg;
  for (int64_t i = 0; i < n; ++i) {
    switch (fn) {
      case 0: cw_sincos(x[i], &out[2 * i], &out[2 * i + 1]); break;
      case 1: {
        float s, c;
        cw_sincos((float)x[i], &s, &c);
        out[2 * i] = s;
        out[2 * i + 1] = c;
        break;
      }
      case 2: {
        v2f s, c;
        Prec<v2f>::sincos_(v2f{(float)x[i], (float)-x[i]}, &s, &c);
        out[2 * i] = s.x;
        out[2 * i + 1] = c.x;
        if (s.y != -s.x || c.y != c.x) return -2;  // the halves are independent and symmetric
        break;
      }
      case 3: out[i] = atan2_upper((float)y[i], (float)x[i]); break;
      case 4: {
        const v2f r = atan2_upper(v2f{(float)y[i], (float)y[i]}, v2f{(float)x[i], (float)x[i]});
        if (r.x != r.y) return -2;
        out[i] = r.x;
        break;
      }
      case 5:
      case 6: {
        double s = std::sin(y[i]), c = std::cos(y[i]);
        out[4 * i] = s;
        out[4 * i + 1] = c;
        for (int k = 0; k < Trig<double>::kResync; ++k) {
          if (fn == 5)
            Trig<double>::step(x[i], s, c);
          else
            Trig<double>::step_addition(x[i], s, c);
        }
        out[4 * i + 2] = s;
        out[4 * i + 3] = c;
        break;
      }
      default: return -1;
    }
  }
  return 0;
}

// The SE(3) log / exp evaluators over arrays, in the instantiations the kernels
// use (tests/test_se3.py).  M [n,12] = R row-major, then p; out [n,6] = [v; w]
// ([n,12] for exp6, whose xi = M[12 i .. 12 i + 6)).
//   fn 0: log6<double> (ikg_log6_batch f64, the controller's err)
//      1: log6<float> (ikg_log6_batch f32; inputs cast)
//      2: log6<double, true> (SE3.Interpolate)        3: exp6<double>
//      4: log6_iter<double>, no tracker
//      5: log6_iter<double> (quad loop)                6: log6_iter<double, true> (pair loop)
//      7: log6_iter<double, true, true> (pair loop, z-aligned targets: its sums uncontracted)
//         5-7 with a tracker.  prev == NULL: a resync update (the tracker zero-initialised, as
//         update 0 finds it).  prev [n,12]: the tracker filled by a resync update on prev[i],
//         then M[i] with resync = false.  fn + 10 (15-17): the rows are ONE chain: a resync
//         update on prev[0 .. 12), then M[0], M[1], ... in turn with resync = false.
//      8: log6_iter<float, true> (pair fp32 loop)
//      9: log6_iter<v2f> (packed loop), both halves fed the row: -2 if they differ
template <bool COLD, bool ROW3>
static void emu_se3_tracked(bool chain, int64_t n, const double* M, const double* prev, double* out) {
  using namespace ikg;
  ThetaTrack<double> tk{};
  double e[6];
  for (int64_t i = 0; i < n; ++i) {
    if (prev && (!chain || i == 0)) {
      tk = ThetaTrack<double>{};
      log6_iter<double, COLD, ROW3>(prev + 12 * i, prev + 12 * i + 9, e, &tk, true);
    } else if (!prev) {
      tk = ThetaTrack<double>{};
    }
    log6_iter<double, COLD, ROW3>(M + 12 * i, M + 12 * i + 9, out + 6 * i, &tk, prev == nullptr);
  }
}

extern "C" int ikg_emu_se3(int fn, int64_t n, const double* M, const double* prev, double* out) {
  using namespace ikg;
  const bool chain = fn >= 15 && fn <= 17;
  if (chain && !prev) return -1;
  switch (chain ? fn - 10 : fn) {
    case 5: emu_se3_tracked<false, false>(chain, n, M, prev, out); return 0;
    case 6: emu_se3_tracked<true, false>(chain, n, M, prev, out); return 0;
    case 7: emu_se3_tracked<true, true>(chain, n, M, prev, out); return 0;
    default: break;
  }
  for (int64_t i = 0; i < n; ++i) {
    const double* Mi = M + 12 * i;
    double* o = out + 6 * i;
    float Mf[12], ef[6];
    for (int k = 0; k < 12; ++k) Mf[k] = (float)Mi[k];
    switch (fn) {
      case 0: log6<double>(Mi, Mi + 9, o); break;
      case 1:
        log6<float>(Mf, Mf + 9, ef);
        for (int k = 0; k < 6; ++k) o[k] = ef[k];
        break;
      case 2: log6<double, true>(Mi, Mi + 9, o); break;
      case 3: exp6<double>(Mi, out + 12 * i, out + 12 * i + 9); break;
      case 4: log6_iter<double>(Mi, Mi + 9, o); break;
      case 8:
        log6_iter<float, true>(Mf, Mf + 9, ef);
        for (int k = 0; k < 6; ++k) o[k] = ef[k];
        break;
      case 9: {
        v2f Mv[12], ev[6];
        for (int k = 0; k < 12; ++k) Mv[k] = v2f{Mf[k], Mf[k]};
        log6_iter<v2f>(Mv, Mv + 9, ev);
        for (int k = 0; k < 6; ++k) {
          const float a = ev[k].x, b = ev[k].y;
          if (std::memcmp(&a, &b, sizeof(float)) != 0) return -2;
          o[k] = a;
        }
        break;
      }
      default: return -1;
    }
  }
  return 0;
}

// What every dynamics entry below starts with: the inertias pass
// ikg_model_set_inertia's checks (else null) and the joint and inertia tables
// are built into this thread's storage.
template <typename T>
struct EmuTables {
  ikg::KModel<T> m;
  ikg::KInertia<T> in;
};
template <typename T>
const EmuTables<T>* emu_tables(const ikg_model_desc* d, const ikg_inertia_desc* id) {
  const char* why = "";
  if (ikg::check_inertia_desc(*id, d->nq, &why) >= 0) return nullptr;
  static thread_local EmuTables<T> t;
  ikg::build_kmodel<T>(*d, t.m);
  ikg::build_kinertia<T>(*d, *id, t.in);
  return &t;
}

// ikg_dynamics_batch on the CPU: the per-body functions of ikg_dynamics.hpp in
// the kernel's order (tests/test_dynamics.py).  v and every output may be NULL.
template <typename T>
int emu_dyn(const ikg_model_desc* d, const ikg_inertia_desc* id, const void* q, const void* v, int64_t B, void* M,
            void* nle, void* g) {
  const EmuTables<T>* t = emu_tables<T>(d, id);
  if (!t) return -1;
  const int nq = d->nq;
  for (int64_t i = 0; i < B; ++i)
    ikg::dynamics_state<T>(t->m, t->in, (const T*)q + nq * i, v ? (const T*)v + nq * i : nullptr,
                           M ? (T*)M + (int64_t)nq * nq * i : nullptr, nle ? (T*)nle + nq * i : nullptr,
                           g ? (T*)g + nq * i : nullptr);
  return 0;
}

extern "C" int ikg_emu_dynamics(const ikg_model_desc* d, const ikg_inertia_desc* id, int dtype, const void* q,
                                const void* v, int64_t B, void* M, void* nle, void* g) {
  return dtype == IKG_F64 ? emu_dyn<double>(d, id, q, v, B, M, nle, g) : emu_dyn<float>(d, id, q, v, B, M, nle, g);
}

// The solve of ikg_control_torque_batch on the CPU (fp64): M and nle from
// dynamics_state, then the phases of control_state; the kinematic terms J
// [B,12,nq], dJv, err, derr [B,12] (ikg_frame_kinematics_batch,
// LOCAL_WORLD_ALIGNED) are inputs.  Outputs may be NULL.
extern "C" int ikg_emu_control_torque(const ikg_model_desc* d, const ikg_inertia_desc* id, const double* q,
                                      const double* v, const double* J, const double* dJv, const double* err,
                                      const double* derr, int64_t B, const ikg_control_params* p, double* tau,
                                      double* qdd, double* xdd, double* Lambda, double* fc) {
  const EmuTables<double>* t = emu_tables<double>(d, id);
  if (!t) return -1;
  const ikg::KCtl<double> prm = ikg::make_kctl<double>(*p);
  const int nq = d->nq;
  for (int64_t i = 0; i < B; ++i) {
    double M[ikg::kMaxNq * ikg::kMaxNq], nle[ikg::kMaxNq];
    ikg::dynamics_state<double>(t->m, t->in, q + nq * i, v ? v + nq * i : nullptr, M, nle, nullptr);
    ikg::control_state<double>(nq, prm, M, nle, J + 12 * nq * i, dJv + 12 * i, err + 12 * i, derr + 12 * i,
                               tau ? tau + nq * i : nullptr, qdd ? qdd + nq * i : nullptr,
                               xdd ? xdd + 12 * i : nullptr, Lambda ? Lambda + 72 * i : nullptr,
                               fc ? fc + 12 * i : nullptr);
  }
  return 0;
}

// ---------------------------------------------------------------- closed-loop rollout on the CPU
// The kinematic terms of one state (J [12,nq], dJ v, e, e' [12],
// LOCAL_WORLD_ALIGNED) in the frame-kinematics kernel's point-velocity form
//   J_k = [a_k x (p - o_k); a_k],  dJ_k = [a'_k x (p - o_k) + a_k x (p' - o'_k); a'_k],  a'_k = w_parent x a_k
// walked over the tree tables (jR / jt / jaxis / jparent).  The kernel's chain
// functions are device-only and specialised per model class, so this is a
// restatement of them, not the same code: an emulated rollout agrees with the
// GPU to rounding, not to the bit.  Everything after the kinematic terms runs
// the shared phase functions of ikg_dynamics.hpp.
namespace {

template <typename T>
struct EmuHand {
  T R[9], p[3], pd[3], w[3];
};

template <typename T>
void emu_frame_pass(const ikg::KModel<T>& m, const T* q, const T* v, EmuHand<T> hand[2], T* J, T* dJv) {
  using namespace ikg;
  const int nq = m.nq;
  T R[kMaxNq][9], o[kMaxNq][3], od[kMaxNq][3], w[kMaxNq][3], a[kMaxNq][3], ad[kMaxNq][3];
  for (int i = 0; i < nq; ++i) {
    const int p = m.jparent[i];
    T Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, op[3] = {0, 0, 0}, odp[3] = {0, 0, 0}, wp[3] = {0, 0, 0};
    if (p >= 0) {
      std::memcpy(Rp, R[p], sizeof(Rp));
      std::memcpy(op, o[p], sizeof(op));
      std::memcpy(odp, od[p], sizeof(odp));
      std::memcpy(wp, w[p], sizeof(wp));
    }
    T d[3], wd[3], s, c;
    matvec3(Rp, m.jt[i], d);
    dcross(wp, d, wd);
    matmul3(Rp, m.jR[i], R[i]);
    column(R[i], m.jaxis[i], a[i]);
    cw_sincos(q[i], &s, &c);
    rotate_axis(R[i], m.jaxis[i], s, c);
    dcross(wp, a[i], ad[i]);
    for (int k = 0; k < 3; ++k) {
      o[i][k] = op[k] + d[k];
      od[i][k] = odp[k] + wd[k];
      w[i][k] = wp[k] + a[i][k] * (v ? v[i] : T(0));
    }
  }
  if (J)
    for (int i = 0; i < 12 * nq; ++i) J[i] = T(0);
  for (int h = 0; h < 2; ++h) {
    const int j = m.arm_q[h][kArmDof - 1];
    EmuHand<T>& f = hand[h];
    T d[3], wd[3];
    matvec3(R[j], m.hand_t[h], d);
    dcross(w[j], d, wd);
    matmul3(R[j], m.hand_R[h], f.R);
    for (int k = 0; k < 3; ++k) {
      f.p[k] = o[j][k] + d[k];
      f.pd[k] = od[j][k] + wd[k];
      f.w[k] = w[j][k];
    }
    if (!J) continue;
    int chain[kMaxNq], n = 0;
    for (int k = j; k >= 0; k = m.jparent[k]) chain[n++] = k;
    T acc[6] = {0, 0, 0, 0, 0, 0};
    for (int c = n - 1; c >= 0; --c) {  // root first, as the kernel accumulates dJ v
      const int k = chain[c];
      T r[3], rd[3], lin[3], t1[3], t2[3];
      for (int i = 0; i < 3; ++i) {
        r[i] = f.p[i] - o[k][i];
        rd[i] = f.pd[i] - od[k][i];
      }
      dcross(a[k], r, lin);
      dcross(ad[k], r, t1);
      dcross(a[k], rd, t2);
      for (int i = 0; i < 3; ++i) {
        J[(6 * h + i) * nq + k] = lin[i];
        J[(6 * h + 3 + i) * nq + k] = a[k][i];
        acc[i] += (t1[i] + t2[i]) * (v ? v[k] : T(0));
        acc[3 + i] += ad[k][i] * (v ? v[k] : T(0));
      }
    }
    for (int i = 0; i < 6; ++i) dJv[6 * h + i] = acc[i];
  }
}

template <typename T>
void emu_frame_terms(const ikg::KModel<T>& m, const T* q, const T* v, const T* qd, const T* vd, T* J, T* dJv, T* err,
                     T* derr) {
  using namespace ikg;
  EmuHand<T> f[2], fd[2];
  emu_frame_pass(m, q, v, f, J, dJv);
  emu_frame_pass(m, qd, vd, fd, (T*)nullptr, (T*)nullptr);
  for (int h = 0; h < 2; ++h) {
    T Re[9], zero[3] = {0, 0, 0}, lg[6];
    matmul3_nt(fd[h].R, f[h].R, Re);
    log6(Re, zero, lg);
    for (int i = 0; i < 3; ++i) {
      err[6 * h + i] = fd[h].p[i] - f[h].p[i];
      err[6 * h + 3 + i] = lg[3 + i];
      derr[6 * h + i] = fd[h].pd[i] - f[h].pd[i];
      derr[6 * h + 3 + i] = fd[h].w[i] - f[h].w[i];
    }
  }
}

bool emu_curve_ok(const ikg_bezier* c) {
  return c && c->points && c->n_points >= 2 && c->n_points <= ikg::kMaxBezier && c->t_max > c->t_min;
}

}  // namespace

// ikg_frame_kinematics_batch's J, dJ v, err, derr (LOCAL_WORLD_ALIGNED, fp64) by the restatement above
extern "C" int ikg_emu_frame_terms(const ikg_model_desc* d, const double* q, const double* v, const double* qd,
                                   const double* vd, int64_t B, double* J, double* dJv, double* err, double* derr) {
  static thread_local ikg::KModel<double> m;
  ikg::build_kmodel<double>(*d, m);
  const int nq = d->nq;
  for (int64_t i = 0; i < B; ++i)
    emu_frame_terms<double>(m, q + nq * i, v ? v + nq * i : nullptr, qd + nq * i, vd ? vd + nq * i : nullptr,
                            J + 12 * nq * i, dJv + 12 * i, err + 12 * i, derr + 12 * i);
  return 0;
}

// ikg_forward_dynamics_batch on the CPU: nle of dynamics_state, M about each
// joint's own origin (inertia_matrix_local_state), then the forward-dynamics kernel's phases
extern "C" int ikg_emu_forward_dynamics(const ikg_model_desc* d, const ikg_inertia_desc* id, const double* q,
                                        const double* v, const double* tau, int64_t B, double* qdd) {
  const EmuTables<double>* t = emu_tables<double>(d, id);
  if (!t) return -1;
  const int nq = d->nq;
  for (int64_t i = 0; i < B; ++i) {
    double M[ikg::kMaxNq * ikg::kMaxNq], nle[ikg::kMaxNq];
    ikg::dynamics_state<double>(t->m, t->in, q + nq * i, v ? v + nq * i : nullptr, nullptr, nle, nullptr);
    ikg::inertia_matrix_local_state<double>(t->m, t->in, q + nq * i, M);
    ikg::forward_dynamics_state<double>(nq, M, nle, tau + nq * i, qdd + nq * i);
  }
  return 0;
}

// ikg_bezier_eval_batch with host pointers on the CPU (bezier_eval); -1 where the entry returns IKG_EINVAL
extern "C" int ikg_emu_bezier(const double* points, int32_t n_points, int32_t dim, double t_min, double t_max,
                              double mult, const double* times, int64_t K, double* out) {
  const ikg_bezier c{points, n_points, t_min, t_max, mult};
  if (!emu_curve_ok(&c) || dim < 1 || dim > IKG_MAX_NQ) return -1;
  for (int64_t k = 0; k < K; ++k)
    if (!(times[k] >= t_min && times[k] <= t_max)) return -1;
  double bc[ikg::kMaxBezier];
  ikg::bezier_coeffs(n_points, bc);
  const ikg::KBezier<double> kb{points, bc, n_points, dim, t_min, t_max, mult};
  for (int64_t k = 0; k < K; ++k)
    for (int j = 0; j < dim; ++j) out[k * dim + j] = ikg::bezier_eval(kb, times[k], j);
  return 0;
}

// ikg_control_rollout on the CPU: per state and tick the kinematic terms
// (above), dynamics_state and control_step_state, the clock and the curves.
// State i reads its control points at points + i stride (0 = one shared pair).
namespace {

int emu_rollout(const ikg_model_desc* d, const ikg_inertia_desc* id, const double* q0, const double* v0,
                const double* t0, int64_t B, const ikg_bezier* bq, const ikg_bezier* bv, int64_t stride_q,
                int64_t stride_v, const ikg_rollout_params* p, const ikg_rollout_out* out) {
  const EmuTables<double>* tb = emu_tables<double>(d, id);
  if (!tb) return -1;
  if (!emu_curve_ok(bq) || !emu_curve_ok(bv) || p->ticks < 0 || p->record_every < 0) return -1;
  if ((out->q_hist || out->v_hist || out->tau_hist) && p->record_every == 0) return -1;
  const ikg::KCtl<double> prm = ikg::make_kctl<double>(p->control);
  const int nq = d->nq;
  double bcq[ikg::kMaxBezier], bcv[ikg::kMaxBezier];
  ikg::bezier_coeffs(bq->n_points, bcq);
  ikg::bezier_coeffs(bv->n_points, bcv);
  const int64_t every = p->record_every, R = every > 0 ? p->ticks / every : 0;
  for (int64_t i = 0; i < B; ++i) {
    const ikg::KBezier<double> cq{bq->points + i * stride_q, bcq, bq->n_points, nq, bq->t_min, bq->t_max, bq->mult};
    const ikg::KBezier<double> cv{bv->points + i * stride_v, bcv, bv->n_points, nq, bv->t_min, bv->t_max, bv->mult};
    double q[ikg::kMaxNq], v[ikg::kMaxNq], qd[ikg::kMaxNq], vd[ikg::kMaxNq], tau[ikg::kMaxNq];
    double t = t0 ? t0[i] : bq->t_min;
    for (int j = 0; j < nq; ++j) {
      q[j] = q0[nq * i + j];
      v[j] = v0 ? v0[nq * i + j] : 0.0;
    }
    for (int64_t k = 0; k <= p->ticks; ++k) {
      for (int j = 0; j < nq; ++j) {
        qd[j] = ikg::bezier_eval(cq, ikg::bezier_clamp(cq, t), j);
        vd[j] = ikg::bezier_eval(cv, ikg::bezier_clamp(cv, t), j);
      }
      if (k == p->ticks) break;
      double M[ikg::kMaxNq * ikg::kMaxNq], nle[ikg::kMaxNq], J[12 * ikg::kMaxNq], dJv[12], e[12], ed[12];
      emu_frame_terms<double>(tb->m, q, v, qd, vd, J, dJv, e, ed);
      ikg::dynamics_state<double>(tb->m, tb->in, q, v, M, nle, nullptr);
      ikg::control_step_state<double>(nq, prm, M, nle, J, dJv, e, ed, p->dt_sim, q, v, tau);
      t += p->dt_traj;
      if (R && (k + 1) % every == 0) {
        const int64_t h = (i * R + (k + 1) / every - 1) * nq;
        for (int j = 0; j < nq; ++j) {
          if (out->q_hist) ((double*)out->q_hist)[h + j] = q[j];
          if (out->v_hist) ((double*)out->v_hist)[h + j] = v[j];
          if (out->tau_hist) ((double*)out->tau_hist)[h + j] = tau[j];
        }
      }
    }
    for (int j = 0; j < nq; ++j) {
      if (out->q) ((double*)out->q)[nq * i + j] = q[j];
      if (out->v) ((double*)out->v)[nq * i + j] = v[j];
    }
    if (out->t) ((double*)out->t)[i] = t;
  }
  return 0;
}

}  // namespace

extern "C" int ikg_emu_control_rollout(const ikg_model_desc* d, const ikg_inertia_desc* id, const double* q0,
                                       const double* v0, const double* t0, int64_t B, const ikg_bezier* bq,
                                       const ikg_bezier* bv, const ikg_rollout_params* p,
                                       const ikg_rollout_out* out) {
  return emu_rollout(d, id, q0, v0, t0, B, bq, bv, 0, 0, p, out);
}

// ikg_control_rollout_curves with host pointers on the CPU
extern "C" int ikg_emu_control_rollout_curves(const ikg_model_desc* d, const ikg_inertia_desc* id, const double* q0,
                                              const double* v0, const double* t0, int64_t B,
                                              const ikg_bezier_set* sq, const ikg_bezier_set* sv,
                                              const ikg_rollout_params* p, const ikg_rollout_out* out) {
  if (!sq || !sv) return -1;
  const ikg_bezier bq{(const double*)sq->points, sq->n_points, sq->t_min, sq->t_max, sq->mult};
  const ikg_bezier bv{(const double*)sv->points, sv->n_points, sv->t_min, sv->t_max, sv->mult};
  return emu_rollout(d, id, q0, v0, t0, B, &bq, &bv, (int64_t)sq->n_points * d->nq, (int64_t)sv->n_points * d->nq, p,
                     out);
}

// ---------------------------------------------------------------- Bezier trajectory fit on the CPU
// ikg_bezier_fit_batch: the phases of ikg_fit.hpp with a loop as their executor.
// -1 where a host-pointer call of the entry returns IKG_EINVAL for its
// parameters; a path whose count is out of range gets the kernel's answer
// (status 1, cost NaN, points untouched).
namespace {

struct HostItems {
  template <typename F>
  void operator()(int count, F&& fn) {
    for (int i = 0; i < count; ++i) fn(i);
  }
};

}  // namespace

extern "C" int ikg_emu_bezier_fit(const double* q0, const double* q1, const double* y, const int64_t* offsets,
                                  int64_t B, int32_t dim, const ikg_fit_params* prm, double* points, double* vpoints,
                                  double* apoints, double* cost, int32_t* status) {
  if (!prm || dim < 1 || dim > IKG_MAX_NQ || prm->degree < ikg::kFitMinDegree || prm->degree > ikg::kFitMaxDegree)
    return -1;
  if (!(prm->total_time > 0) || !std::isfinite(prm->total_time) || !(prm->ridge >= 0) || !std::isfinite(prm->ridge))
    return -1;
  const int d = prm->degree;
  double bc[ikg::kFitMaxDegree + 1];
  ikg::bezier_coeffs(d + 1, bc);
  std::vector<double> ws(ikg::fit_ws_len(d, dim));
  ikg::FitWs w;
  ikg::fit_ws_bind(ws.data(), d, dim, w);
  HostItems ex;
  for (int64_t p = 0; p < B; ++p) {
    const int64_t n = offsets[p + 1] - offsets[p];
    if (!ikg::fit_count_ok(n, d, prm->ridge)) {
      status[p] = 1;
      ikg::fit_store_nan(cost + p);
      continue;
    }
    const ikg::FitPath f{q0 + p * dim, q1 + p * dim, y + offsets[p] * dim, (int)n, dim, d, prm->ridge,
                         prm->total_time, bc};
    cost[p] = ikg::bezier_fit_path(f, w, ex, points + p * (d + 1) * dim, vpoints ? vpoints + p * d * dim : nullptr,
                                   apoints ? apoints + p * (d - 1) * dim : nullptr);
    status[p] = 0;
  }
  return 0;
}

// ---------------------------------------------------------------- planner primitives on the CPU
// ikg_se3_interpolate_batch with host pointers: the kernel's se3_interpolate (tests/test_rrt.py)
extern "C" int ikg_emu_se3_interpolate(const double* A, const double* B, const double* alpha, int64_t C, double* out) {
  for (int64_t i = 0; i < C; ++i) ikg::se3_interpolate(A + 12 * i, B + 12 * i, alpha[i], out + 12 * i);
  return 0;
}

// ikg_nearest_batch with host pointers: the kernel's per-row distance and its
// argmin rule, combined in the kernel's order (64 lanes striding the rows, then
// the butterfly over the lanes); -1 where the entry returns IKG_EINVAL
extern "C" int ikg_emu_nearest(const double* nodes, int64_t cap, const int32_t* counts, const double* queries,
                               int32_t nq, int64_t P, int32_t* index, double* dist) {
  if (cap < 0 || nq < 1) return -1;
  for (int64_t p = 0; p < P; ++p) {
    if (counts[p] < 0 || counts[p] > cap) return -1;
    double d2[64];
    int best[64];
    for (int lane = 0; lane < 64; ++lane) {
      d2[lane] = DBL_MAX;
      best[lane] = -1;
      for (int64_t r = lane; r < counts[p]; r += 64) {
        const double d = ikg::row_dist2(nodes + (p * cap + r) * nq, queries + p * nq, nq);
        if (ikg::nearest_takes(d2[lane], best[lane], d, (int)r)) {
          d2[lane] = d;
          best[lane] = (int)r;
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      double od[64];
      int ob[64];
      for (int lane = 0; lane < 64; ++lane) {
        od[lane] = d2[lane ^ off];
        ob[lane] = best[lane ^ off];
      }
      for (int lane = 0; lane < 64; ++lane)
        if (ikg::nearest_takes(d2[lane], best[lane], od[lane], ob[lane])) {
          d2[lane] = od[lane];
          best[lane] = ob[lane];
        }
    }
    index[p] = best[0];
    dist[p] = best[0] >= 0 ? std::sqrt(d2[0]) : 0.0;
  }
  return 0;
}

// ikg_project_paths with host pointers on the CPU: the entry's step loop
// (projection_host_steps, the zeroed outputs, prepare / solve / commit per step)
// with the kernels' per-chain functions (project_prepare_chain,
// project_commit_chain) run over the chains in turn and emu<double> as the
// collision solve between them (p->check_collision as the caller sets it).  -1
// where the entry returns IKG_EINVAL.  steps_run (may be NULL): the steps the
// loop ran.  tests/test_projection.py.
extern "C" int ikg_emu_project_paths(const ikg_model_desc* d, const ikg_collision_desc* cd, const double* q_curr,
                                     const double* cube_curr, const double* cube_rand, int64_t C, double step_size,
                                     int32_t max_nodes, const int32_t* geoms, int32_t n_geoms, const ikg_params* p,
                                     double* robot_path, double* cube_path, int32_t* n_nodes, int32_t* status,
                                     int32_t* steps_run) {
  if (!d || !cd || !p || C < 0 || !(step_size > 0) || !std::isfinite(step_size) || max_nodes < 1) return -1;
  if (n_geoms < 1 || n_geoms > IKG_MAX_GEOMS || !geoms) return -1;
  static thread_local ikg::KCollision<double> kc;
  ikg::build_kcollision<double>(*cd, kc);
  if (kc.target_geom < 0) return -1;
  ikg::ProjectArgs a{};
  a.geoms.n = n_geoms;
  for (int32_t k = 0; k < n_geoms; ++k) {
    if (geoms[k] < 0 || geoms[k] >= kc.n_geoms || geoms[k] == kc.target_geom) return -1;
    a.geoms.g[k] = geoms[k];
  }
  if (steps_run) *steps_run = 0;
  if (C == 0) return 0;
  int64_t bad = 0;
  const int64_t n_steps = ikg::projection_host_steps(cube_curr, cube_rand, C, step_size, max_nodes, &bad);
  if (n_steps < 0) return -1;
  const int nq = d->nq;
  std::vector<double> targets(12 * C), q0(nq * C), q(nq * C), err(2 * C);
  std::vector<int32_t> iters(C), aux(2 * C);
  std::vector<uint8_t> conv(C);
  a.q_curr = q_curr;
  a.cube_curr = cube_curr;
  a.cube_rand = cube_rand;
  a.C = C;
  a.nq = nq;
  a.max_nodes = max_nodes;
  a.step_size = step_size;
  a.robot_path = robot_path;
  a.cube_path = cube_path;
  a.n_nodes = n_nodes;
  a.status = status;
  a.targets = targets.data();
  a.q0 = q0.data();
  a.q = q.data();
  a.conv = conv.data();
  a.steps = aux.data();
  a.free_ = aux.data() + C;
  std::memset(robot_path, 0, sizeof(double) * nq * max_nodes * C);
  std::memset(cube_path, 0, sizeof(double) * 12 * max_nodes * C);
  chest_mismatch = 0;
  for (int64_t step = 1; step <= std::max<int64_t>(n_steps, 1); ++step) {
    for (int64_t i = 0; i < C; ++i) ikg::project_prepare_chain(&kc, a, i, (int)step);
    if (step > n_steps) break;  // max_nodes = 1: the chains are cut at their first row
    emu<double>(d, targets.data(), q0.data(), nq, C, p, q.data(), conv.data(), iters.data(), err.data(), nullptr, 0, cd);
    for (int64_t i = 0; i < C; ++i) ikg::project_commit_chain(a, i, (int)step);
    if (steps_run) *steps_run = (int32_t)step;
  }
  return chest_mismatch ? -3 : 0;
}

// ---------------------------------------------------------------- trajectory check on the CPU
// ikg_trajectory_check_batch with host pointers: per sample the functions of
// ikg_trajcheck.hpp, the check stages run serially (emu_collide's, with the
// lowest colliding pair kept) and pair_distance over pair_idx as
// ikg_distance_kernel forms it, then partial_add over the samples in order
// (what the waves' partials fold to whatever the chunking).  -1 where the entry
// returns IKG_EINVAL.  tests/test_trajcheck.py.
extern "C" int ikg_emu_trajectory_check(const ikg_model_desc* d, const ikg_collision_desc* cd,
                                        const ikg_bezier_set* curves, int64_t B, const double* cube_fixed,
                                        const int32_t* pair_idx, int32_t n_pairs, const ikg_trajcheck_params* p,
                                        const ikg_trajcheck_out* out) {
  using namespace ikg;
  if (!d || !cd || !curves || !p || !out || B < 0) return -1;
  const ikg_bezier one{(const double*)curves->points, curves->n_points, curves->t_min, curves->t_max, curves->mult};
  if (B > 0 && !emu_curve_ok(&one)) return -1;
  if (curves->n_points < 2 || curves->n_points > kMaxBezier || !(curves->t_max > curves->t_min)) return -1;
  if (p->samples < 2 || p->samples_per_wave < 0) return -1;
  if (p->cube_mode != IKG_CUBE_CARRIED && p->cube_mode != IKG_CUBE_FIXED) return -1;
  if (p->cube_mode == IKG_CUBE_FIXED && B > 0 && !cube_fixed) return -1;
  if (n_pairs < 0 || (n_pairs > 0 && !pair_idx)) return -1;
  KModel<double> m;
  build_kmodel<double>(*d, m);
  static thread_local KCollision<double> kc;
  build_kcollision<double>(*cd, kc);
  if (kc.target_geom < 0) return -1;
  for (int32_t k = 0; k < n_pairs; ++k)
    if (pair_idx[k] < 0 || pair_idx[k] >= kc.n_pairs) return -1;
  const int nq = d->nq, S = p->samples, n = curves->n_points;
  const bool fixed = p->cube_mode == IKG_CUBE_FIXED;
  const bool want_d = n_pairs > 0 && (out->min_clearance || out->arg_clearance || out->clearance);
  double bc[kMaxBezier];
  bezier_coeffs(n, bc);
  const TrajFoldOut o{out->first_collision,        out->first_pair,    out->n_collision,
                      (double*)out->min_clearance, out->arg_clearance, (double*)out->max_grasp,
                      out->arg_grasp,              (double*)out->max_limit, out->arg_limit};
  for (int64_t b = 0; b < B; ++b) {
    const KBezier<double> kb{(const double*)curves->points + b * n * nq, bc, n, nq, curves->t_min, curves->t_max,
                             curves->mult};
    TrajPartial part;
    partial_init(part);
    for (int k = 0; k < S; ++k) {
      const int64_t row = b * S + k;
      double q[kMaxNq], L[kMaxNq][12], F[kMaxNq][12], P[kMaxGeoms][12], eff[2][12], tgt[12];
      const double t = trajcheck_time(curves->t_min, curves->t_max, S, k);
      double lim = 0.0;
      for (int j = 0; j < nq; ++j) {
        q[j] = bezier_eval(kb, t, j);
        double sn, cs;
        Prec<double>::sincos_(q[j], &sn, &cs);
        joint_local(&m, j, sn, cs, L[j]);
        lim = fmax(lim, limit_excess(&m, j, q[j]));
      }
      for (int j = 0; j < nq; ++j) joint_world(m.jparent, j, L, F[j]);
      for (int h = 0; h < 2; ++h) effector_world(&m, h, F, eff[h]);
      if (fixed)
        for (int i = 0; i < 12; ++i) tgt[i] = cube_fixed[b * 12 + i];
      else
        carried_cube(&m, eff[0], tgt);
      const double gR = grasp_norm(&m, 1, eff[1], tgt);
      const double grasp = fixed ? fmax(grasp_norm(&m, 0, eff[0], tgt), gR) : gR;
      for (int g = 0; g < kc.n_geoms; ++g) geom_world(&kc, g, F, tgt, P[g]);
      int pair = -1;
      for (int i = 0; i < kc.n_pairs && pair < 0; ++i)
        if (pair_hit(&kc, i, P)) pair = i;
      double dmin = kNoClearance;
      if (want_d)
        for (int i = 0; i < n_pairs; ++i) {
          const int ga = kc.pairs[pair_idx[i]][0], gb = kc.pairs[pair_idx[i]][1];
          dmin = fmin(dmin, pair_distance(pair_shape(&kc, ga, P), pair_shape(&kc, gb, P)));
        }
      partial_add(part, k, pair >= 0, pair, want_d, dmin, grasp, lim);
      if (out->collision) out->collision[row] = pair >= 0 ? 1 : 0;
      if (out->clearance) ((double*)out->clearance)[row] = dmin;
      if (out->grasp) ((double*)out->grasp)[row] = grasp;
      if (out->limit) ((double*)out->limit)[row] = lim;
      if (out->cube)
        for (int i = 0; i < 12; ++i) ((double*)out->cube)[row * 12 + i] = tgt[i];
    }
    fold_store(o, b, part);
  }
  return 0;
}

// ---------------------------------------------------------------- trajectory dynamics on the CPU
// ikg_trajectory_dynamics_batch with host pointers: the derivative control
// points and multipliers as the launcher and the kernel form them, bezier_eval
// per joint, inverse_dynamics_state, then dynpartial_add over the samples in
// order, joints ascending (what the waves' partials fold to whatever the
// chunking).  -1 where the entry returns IKG_EINVAL.  tests/test_trajdyn.py.
extern "C" int ikg_emu_trajectory_dynamics(const ikg_model_desc* d, const ikg_inertia_desc* id,
                                           const ikg_bezier_set* curves, int64_t B, const ikg_trajdyn_params* p,
                                           const ikg_trajdyn_out* out) {
  using namespace ikg;
  if (!d || !id || !curves || !p || !out || B < 0) return -1;
  if (B > 0 && !curves->points) return -1;
  if (curves->n_points < kTrajDynMinPoints || curves->n_points > kMaxBezier || !(curves->t_max > curves->t_min))
    return -1;
  if (p->samples < 2 || p->samples_per_wave < 0) return -1;
  const int nq = d->nq, S = p->samples, n = curves->n_points;
  for (int j = 0; j < nq; ++j)
    if (!(p->velocity_limit[j] > 0) || !(p->effort_limit[j] > 0) || !std::isfinite(p->velocity_limit[j]) ||
        !std::isfinite(p->effort_limit[j]))
      return -1;
  const EmuTables<double>* t = emu_tables<double>(d, id);
  if (!t) return -1;
  static thread_local TrajDynArgs a;
  a.n_points = n;
  a.t_min = curves->t_min;
  a.t_max = curves->t_max;
  a.mult = curves->mult;
  trajdyn_curve_setup(a);
  const TrajDynFoldOut o{(double*)out->speed_scale, out->arg_speed,  (double*)out->torque_use,
                         out->arg_torque_use,       (double*)out->static_use, out->arg_static,
                         out->n_static,             (double*)out->torque_scale, out->arg_torque_scale};
  std::vector<double> Pv((size_t)(n - 1) * nq), Pa((size_t)(n - 2) * nq);
  for (int64_t b = 0; b < B; ++b) {
    const double* Pq = (const double*)curves->points + b * n * nq;
    for (int i = 0; i < (n - 1) * nq; ++i) Pv[i] = bezier_derivative_point(Pq, n, nq, i / nq, i % nq);
    for (int i = 0; i < (n - 2) * nq; ++i) Pa[i] = bezier_derivative_point(Pv.data(), n - 1, nq, i / nq, i % nq);
    const KBezier<double> cq{Pq, a.bc[0], n, nq, a.t_min, a.t_max, a.mult};
    const KBezier<double> cv{Pv.data(), a.bc[1], n - 1, nq, a.t_min, a.t_max, a.mult_v};
    const KBezier<double> ca{Pa.data(), a.bc[2], n - 2, nq, a.t_min, a.t_max, a.mult_a};
    TrajDynPartial part;
    dynpartial_init(part);
    for (int k = 0; k < S; ++k) {
      const double tk = trajcheck_time(a.t_min, a.t_max, S, k);
      double q[kMaxNq], v[kMaxNq], acc[kMaxNq], tau[kMaxNq], g[kMaxNq];
      for (int j = 0; j < nq; ++j) {
        q[j] = bezier_eval(cq, tk, j);
        v[j] = bezier_eval(cv, tk, j);
        acc[j] = bezier_eval(ca, tk, j);
      }
      inverse_dynamics_state<double>(t->m, t->in, q, v, acc, tau, g);
      for (int j = 0; j < nq; ++j) {
        dynpartial_add(part, k, j, v[j], tau[j], g[j], p->velocity_limit[j], p->effort_limit[j]);
        const int64_t at = (b * S + k) * nq + j;
        if (out->tau) ((double*)out->tau)[at] = tau[j];
        if (out->g) ((double*)out->g)[at] = g[j];
      }
    }
    dynfold_store(o, b, part);
  }
  return 0;
}
