// C-ABI of libikgrasp.so (include/ikgrasp.h).
//
// Owns model validation / upload, argument checking, optional host staging
// and kernel dispatch.  No exception or exit crosses the boundary: every
// failure returns a negative code and leaves a message in ikg_last_error().
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "ikg_device.hpp"
#include "ikg_jit.hpp"
#include "ikg_solve.hpp"
#include "ikg_launch.hpp"
#include "ikg_fit.hpp"
#include "ikg_model_build.hpp"
#include "ikg_planner.hpp"
#include "ikg_trajcheck.hpp"
#include "ikgrasp.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(IKG_EHIP, "%s: %s", what, hipGetErrorString(e));
}

void free_slots(std::vector<void*>& slot) {
  for (size_t i = 0; i < slot.size(); ++i)
    if (slot[i]) {
      (void)hipSetDevice((int)i);
      (void)hipFree(slot[i]);
      slot[i] = nullptr;
    }
}

// One kind of table a model carries (joint tree, collision scene, inertias):
// the fp64 and fp32 host tables and their uploads, one slot per device.
template <template <typename> class K>
struct Tables {
  const char* missing;  // the error of a query before the tables were attached
  bool present = false;
  K<double> k64;
  K<float> k32;
  std::vector<void*> dev64, dev32;

  // Upload to `device` once (under the model's lock); the slot is reused after.
  template <typename T>
  int get(std::mutex& mu, int device, const K<T>** out) {
    if (!present) return fail(IKG_EINVAL, "%s", missing);
    constexpr bool d = sizeof(T) == 8;
    std::vector<void*>& slot = d ? dev64 : dev32;
    const void* src = d ? (const void*)&k64 : (const void*)&k32;
    std::lock_guard<std::mutex> lock(mu);
    if ((int)slot.size() <= device) slot.resize(device + 1, nullptr);
    if (!slot[device]) {
      void* p = nullptr;
      hipError_t e = hipMalloc(&p, sizeof(K<T>));
      if (e != hipSuccess) return fail(IKG_ENOMEM, "hipMalloc(model tables): %s", hipGetErrorString(e));
      e = hipMemcpy(p, src, sizeof(K<T>), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "hipMemcpy(model tables)");
      }
      slot[device] = p;
    }
    *out = (const K<T>*)slot[device];
    return IKG_OK;
  }

  // free the uploads (they are made again lazily); callers must not race a launch
  void reset() {
    int prev = -1;
    (void)hipGetDevice(&prev);
    free_slots(dev64);
    free_slots(dev32);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace

struct ikg_model {
  ikg_model_desc desc;
  int spec = ikg::kSpecGeneric;
  std::mutex mu;
  Tables<ikg::KModel> kin{"", true};
  Tables<ikg::KCollision> col{"no collision scene attached (ikg_model_set_collision)"};
  Tables<ikg::KInertia> ine{"no body inertias attached (ikg_model_set_inertia)"};
  // model-specialised pair kernels (ikg_model_specialize): code objects per
  // dtype (0 = f64, 1 = f32), loaded modules per device
  std::vector<char> jit_code[2];
  std::vector<ikg::JitKernels*> jit[2];
  // scratch of solves captured into graphs (ikg_launch.hpp ws_alloc), freed here
  ikg::WsOwner ws;

  template <typename T>
  const ikg::JitKernels* jit_kernels(int device) {
    std::lock_guard<std::mutex> lock(mu);
    const auto& v = jit[sizeof(T) == 8 ? 0 : 1];
    return device < (int)v.size() ? v[device] : nullptr;
  }
};

namespace {

// Select and restore the current device around a call.
struct DeviceGuard {
  int prev = -1;
  int rc = IKG_OK;
  explicit DeviceGuard(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
      rc = hip_fail(e, "hipGetDeviceCount");
      return;
    }
    if (device < 0 || device >= n) {
      rc = fail(IKG_ENODEV, "device %d out of range (%d visible)", device, n);
      return;
    }
    (void)hipGetDevice(&prev);
    e = hipSetDevice(device);
    if (e != hipSuccess) rc = hip_fail(e, "hipSetDevice");
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// The pointers of one call.  With IKG_FLAG_HOST_POINTERS every input and output
// is staged through device scratch that lives until the call returns; without
// it in() and out() hand the caller's device pointers through.
struct Staging {
  struct Out {
    void *host, *dev;
    size_t bytes;
  };
  std::vector<void*> allocs;
  std::vector<Out> outs;
  hipStream_t s;
  bool host;
  int rc = IKG_OK;
  Staging(hipStream_t st, uint32_t flags) : s(st), host(flags & IKG_FLAG_HOST_POINTERS) {}
  ~Staging() {
    for (void* p : allocs) (void)hipFree(p);
  }
  void* alloc(size_t bytes) {
    if (rc) return nullptr;
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes ? bytes : 1);
    if (e != hipSuccess) {
      rc = fail(IKG_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
      return nullptr;
    }
    allocs.push_back(d);
    return d;
  }
  // a device copy of a host array, whatever the flag (the small tables of a call)
  void* upload(const void* p, size_t bytes) {
    void* d = p ? alloc(bytes) : nullptr;
    if (d && bytes) {
      const hipError_t e = hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, s);
      if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync(H2D)");
    }
    return d;
  }
  const void* in(const void* p, size_t bytes) { return host ? upload(p, bytes) : p; }
  // an optional output: the device buffer the kernels write; finish() copies it back
  void* out(void* p, size_t bytes) {
    if (!host || !p) return p;
    void* d = alloc(bytes);
    outs.push_back({p, d, bytes});
    return d;
  }
  // The end of a call whose launches are queued: copy the staged outputs back
  // and wait for them.  `sync`: wait although the call passed device pointers
  // (scratch of this object is still in use by the queued kernels).
  int finish(bool sync = false) {
    for (const Out& o : outs) {
      if (!o.dev || rc) break;
      const hipError_t e = hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, s);
      if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync(D2H)");
    }
    if (rc) return rc;
    if (host || sync) {
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    }
    return IKG_OK;
  }
};

// Problems per wave.  Full 32-problem waves are fastest at every batch size
// measured (B = 4k..131k, fp32/fp64): spreading a small batch over more,
// sparser waves was 1.3-3x SLOWER (profiles/r01/ppw_sweep.txt).
int auto_ppw(int /*device*/, int64_t /*B*/) { return 32; }

// One-wave-per-problem kernels (collision query, pre-screen, continuation,
// distance, best-seed) launch one 64-lane workgroup per unit; HIP caps a grid at
// 2^32 - 1 work items, so a launch holds at most this many waves.
constexpr int64_t kMaxWaves = (int64_t)0xFFFFFFFFu / 64;

int check_params(const ikg_params* p) {
  if (!p) return fail(IKG_EINVAL, "params is NULL");
  if (!(p->eps > 0) || !std::isfinite(p->eps)) return fail(IKG_EINVAL, "eps must be > 0");
  if (!std::isfinite(p->dt)) return fail(IKG_EINVAL, "dt must be finite");
  if (p->max_iters < 0) return fail(IKG_EINVAL, "max_iters must be >= 0");
  if (!(p->lambda >= 0) || !std::isfinite(p->lambda)) return fail(IKG_EINVAL, "lambda must be >= 0");
  if (p->variant != IKG_VARIANT_AUTO && p->variant != IKG_VARIANT_PAIR && p->variant != IKG_VARIANT_PACKED &&
      p->variant != IKG_VARIANT_QUAD)
    return fail(IKG_EINVAL, "variant %d not available in this build", p->variant);
  if (p->problems_per_wave < 0 || p->problems_per_wave > 32)
    return fail(IKG_EINVAL, "problems_per_wave must be in [0, 32]");
  if (p->check_collision != 0 && p->check_collision != 1) return fail(IKG_EINVAL, "check_collision must be 0 or 1");
  return IKG_OK;
}

// Host-pointer inputs are checked for finiteness before staging: the device
// code is compiled with -ffinite-math-only, so a NaN/inf target, q0 row or seed
// would be undefined there.  Device-pointer callers own that contract
// (include/ikgrasp.h "Conventions").
template <typename T>
int check_finite(const void* p, int64_t n, const char* what) {
  const T* x = static_cast<const T*>(p);
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return fail(IKG_EINVAL, "%s[%lld] is not finite", what, (long long)i);
  return IKG_OK;
}

// the [B, width] arrays of a host-pointer call, in the order given; a null (optional) array passes
struct HostArray {
  const void* p;
  int64_t width;
  const char* what;
};
template <typename T>
int check_finite_rows(uint32_t flags, int64_t B, std::initializer_list<HostArray> rows) {
  if (!(flags & IKG_FLAG_HOST_POINTERS)) return IKG_OK;
  for (const HostArray& r : rows)
    if (r.p)
      if (int rc = check_finite<T>(r.p, B * r.width, r.what)) return rc;
  return IKG_OK;
}

// f(T{}) for the element type of `dtype` (checked by the caller)
template <typename F>
int by_dtype(int dtype, F&& f) {
  return dtype == IKG_F64 ? f(double{}) : f(float{});
}

template <typename T>
ikg::KParams<T> kparams(const ikg_params* p) {
  return ikg::make_kparams<T>(p);
}

template <typename T>
int check_variant(const ikg_model* model, const ikg_params* params) {
  if (params->variant == IKG_VARIANT_PACKED && (sizeof(T) != 4 || model->spec != ikg::kSpecNextage || params->lambda > 0))
    return fail(IKG_EINVAL, "variant PACKED needs fp32, a Nextage-class model and lambda = 0");
  if (params->variant == IKG_VARIANT_QUAD && (model->spec != ikg::kSpecNextage || params->lambda > 0))
    return fail(IKG_EINVAL, "variant QUAD needs a Nextage-class model and lambda = 0");
  return IKG_OK;
}

// Records in the batch kernel for the collision continuation (the default
// since round 3: C2 with the collision term 1.62 -> 1.30 ms; IKG_TRAJ_REC=0
// selects the trajectory kernel, which recomputes the updates past the first
// passing iterate).  Its round-2 graph-replay mismatch was the graph memory
// node the records came from (ws_alloc, ikg_launch.hpp).  Up
// to rec_budget() bytes of records per solve.
static bool rec_in_batch() { return ikg::env_flag("IKG_TRAJ_REC", true); }
// Memory of a collision solve (round 6, window checkpoints, ikg_solve.hpp):
//  * checkpoints, one area per problem of a launch (ck_per_problem: 34 slots,
//    17 KB in fp64, 8.7 KB in fp32 at max_iters 1,000: C2 71 MB, C3 570 MB,
//    C4's 131,072-problem fp64 share 2.3 GB).  A batch whose checkpoints exceed
//    the checkpoint budget (16 GiB, IKG_CK_BUDGET_MB) is solved in chunks of
//    equal size that fit, one launch sequence per chunk (fixed slots carry no
//    shared state, so a problem's answer does not depend on the chunking);
//  * the regenerated records of the problems the scan lists, (max_iters + 1)
//    records per problem, for as many problems as the records budget holds
//    (1 GiB, IKG_REC_BUDGET_MB: 6,700 fp64 / 13,400 fp32 problems); the resume
//    kernel and the records scan run in rounds of that many list entries
//    (ikg_collision.hip launch_collide_continue).
// Round 5 held every problem's records (C3 fp32 5.2 GB, the C4 share 21 GB)
// under a 24 GiB budget; the model's pool keeps 1.25 GiB between solves
// (ikg_launch.hpp ws_keep_bytes).
constexpr size_t kRecBudgetMB = 1024, kCkBudgetMB = 16384;
static size_t budget_bytes(const char* name, size_t mb) {
  return std::max<size_t>(1, (size_t)ikg::env_int(name, (long long)mb)) << 20;
}
static size_t rec_budget() { return budget_bytes("IKG_REC_BUDGET_MB", kRecBudgetMB); }
static size_t ck_budget() { return budget_bytes("IKG_CK_BUDGET_MB", kCkBudgetMB); }

// the final record (record layout) fits a checkpoint slot (ikg_solve.hpp kCkSlot)
static bool rec_fits(int nq) {
  return ikg::rec_len(std::max(0, nq - 1 - 2 * ikg::kArmDof)) <= ikg::kCkSlot;
}

// bytes of one problem's regenerated records, and of its checkpoints
template <typename T>
static size_t rec_records_bytes(const ikg_params& params, int nq) {
  const size_t rl = (size_t)ikg::rec_len(std::max(0, nq - 1 - 2 * ikg::kArmDof));
  return sizeof(T) * rl * ((size_t)params.max_iters + 1);
}
template <typename T>
static size_t rec_ck_bytes(const ikg_params& params) {
  return sizeof(T) * (size_t)ikg::ck_per_problem<T>(params.max_iters);
}

// units (problems, or multi-start targets of `per_unit` problems each) per
// launch: all of them when their checkpoints fit the budget, else the fewest
// equal chunks that do (at least one unit)
template <typename T>
static int64_t rec_chunk(const ikg_params& params, int64_t units, int64_t per_unit) {
  const size_t unit_bytes = rec_ck_bytes<T>(params) * (size_t)per_unit;
  const int64_t cap = std::max<int64_t>(1, (int64_t)(ck_budget() / std::max<size_t>(1, unit_bytes)));
  if (units <= cap) return units;
  const int64_t n = (units + cap - 1) / cap;
  return (units + n - 1) / n;
}

// Whether a collision solve is offered records, but for the layout (QUAD
// takes none), which each caller tests its own way: the collision term, the
// compiled Nextage loop (no damping, no model-specialised kernel), records on
// and a final record that fits a checkpoint slot.
static bool records_apply(const ikg_model* model, const ikg_params* params, bool collision, bool jit, int nq) {
  return collision && model->spec == ikg::kSpecNextage && !(params->lambda > 0) && !jit && rec_in_batch() &&
         rec_fits(nq);
}

// Checkpoints and records of the collision continuation for `n` problems (one
// chunk, see solve_batch_t), in `ws`: checkpoints for all n, records for the
// records budget's capacity (rec_slots).  All null when the allocation fails
// (the continuation then runs without them).
template <typename T>
ikg::RecBufs offer_records(ikg::Workspace& ws, const ikg_params& params, int64_t n, int nq, bool* rec_used) {
  const size_t per = rec_records_bytes<T>(params, nq);
  const int64_t slots = std::min<int64_t>(n, std::max<int64_t>(1, (int64_t)(rec_budget() / per)));
  const ikg::RecLayout l(n, slots, per, rec_ck_bytes<T>(params));
  if (ws.alloc(l) != hipSuccess) {
    (void)hipGetLastError();
    return {};
  }
  return {ws.at<void>(l.rec), ws.at<int32_t>(l.rec_n), ws.at<void>(l.ck), rec_used, slots};
}

// chunk [off, off + n) of a batch's arguments (device pointers)
template <typename T>
static ikg::BatchArgs batch_slice(const ikg::BatchArgs& a, int64_t off, int64_t n, int nq) {
  ikg::BatchArgs c = a;
  c.B = n;
  c.targets = (const T*)a.targets + off * 12;
  if (a.q0_stride) c.q0 = (const T*)a.q0 + off * a.q0_stride;
  c.q_out = (T*)a.q_out + off * nq;
  if (a.converged) c.converged = a.converged + off;
  if (a.iters) c.iters = a.iters + off;
  if (a.err_out) c.err_out = (T*)a.err_out + off * 2;
  return c;
}

template <typename T>
int solve_batch_t(ikg_model* model, int device, const void* targets, const void* q0, int64_t q0_stride, int64_t B,
                  const ikg_params* params, void* q_out, uint8_t* converged, int32_t* iters, void* err_out,
                  hipStream_t s, uint32_t flags) {
  if (!ikg::stream_capturing(s)) ikg::ws_drain(&model->ws);  // scratch of destroyed graphs
  const ikg::KModel<T>* dm = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc) return rc;
  const ikg::KCollision<T>* dc = nullptr;
  if (params->check_collision && (rc = model->col.get<T>(model->mu, device, &dc))) return rc;
  const int nq = model->desc.nq;
  if ((rc = check_variant<T>(model, params))) return rc;
  Staging st(s, flags);
  const int64_t q0_rows = q0_stride == 0 ? 1 : B;
  if (st.host) {
    if ((rc = check_finite<T>(targets, 12 * B, "targets"))) return rc;
    for (int64_t r = 0; r < q0_rows; ++r)
      if ((rc = check_finite<T>(static_cast<const T*>(q0) + r * q0_stride, nq, "q0 row"))) return rc;
  }
  ikg::BatchArgs a{st.in(targets, sizeof(T) * 12 * B),
                   st.in(q0, sizeof(T) * (q0_stride * (q0_rows - 1) + nq)),
                   q0_stride,
                   B,
                   st.out(q_out, sizeof(T) * nq * B),
                   (uint8_t*)st.out(converged, B),
                   (int32_t*)st.out(iters, sizeof(int32_t) * B),
                   st.out(err_out, sizeof(T) * 2 * B),
                   32};
  if (st.rc) return st.rc;
  a.ws_owner = &model->ws;
  a.ppw = params->problems_per_wave > 0 ? params->problems_per_wave : auto_ppw(device, B);
  a.variant = params->variant;
  if (dc) {  // the continuation reads and rewrites every per-problem output
    if (!a.converged) a.converged = (uint8_t*)st.alloc(B);
    if (!a.iters) a.iters = (int32_t*)st.alloc(sizeof(int32_t) * B);
    if (!a.err_out) a.err_out = st.alloc(sizeof(T) * 2 * B);
    if (st.rc) return st.rc;
  }
  a.jit = model->jit_kernels<T>(device);
  // collision term, pair layout, Nextage loop: the batch kernel itself records
  // every iterate from the first passing one on, for the continuation's scan
  // (ikg_collision.hip), whatever the q0 layout; the records
  // take (max_iters + 1) x rec_len values per problem, offered up to the budget
  bool rec_used = false;
  ikg::Workspace rec(&model->ws, s, "rec");
  int64_t chunk = B;
  const ikg::KParams<T> kp = kparams<T>(params);
  if (records_apply(model, params, dc != nullptr, a.jit != nullptr, nq) &&
      ikg::resolve_variant<T>(kp, model->spec, a.variant, B, true) != IKG_VARIANT_QUAD) {
    chunk = rec_chunk<T>(*params, B, 1);
    a.recs = offer_records<T>(rec, *params, chunk, nq, &rec_used);
    if (!rec) chunk = B;
    // every chunk runs the layout the whole batch would
    if (chunk < B) a.variant = ikg::resolve_variant<T>(kp, model->spec, a.variant, B, true);
  }
  hipError_t e = hipSuccess;
  for (int64_t off = 0; off < B && e == hipSuccess; off += chunk) {
    const ikg::BatchArgs c = chunk < B ? batch_slice<T>(a, off, std::min(chunk, B - off), nq) : a;
    e = ikg::launch_pair_batch<T>(dm, kp, c, model->spec, s);
    if (e != hipSuccess) return hip_fail(e, "ikg pair kernel launch");
    if (dc) e = ikg::launch_collide_continue<T>(dm, dc, kp, c, model->spec, nq, model->col.k64.n_geoms, s);
  }
  e = rec.finish(e);
  if (e != hipSuccess) return hip_fail(e, "ikg collision continuation launch");
  return st.finish();
}

template <typename T>
int solve_multi_t(ikg_model* model, int device, const void* targets, int64_t T_, const void* seeds, int64_t S,
                  const ikg_params* params, void* q_out, uint8_t* converged, int32_t* iters, void* err_out,
                  int32_t* best_seed, hipStream_t s, uint32_t flags) {
  if (!ikg::stream_capturing(s)) ikg::ws_drain(&model->ws);  // scratch of destroyed graphs
  const ikg::KModel<T>* dm = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc) return rc;
  const int nq = model->desc.nq;
  if ((rc = check_variant<T>(model, params))) return rc;
  const ikg::KCollision<T>* dc = nullptr;
  if (params->check_collision && (rc = model->col.get<T>(model->mu, device, &dc))) return rc;
  Staging st(s, flags);
  if (st.host &&
      ((rc = check_finite<T>(targets, 12 * T_, "targets")) || (rc = check_finite<T>(seeds, nq * S, "seeds"))))
    return rc;
  ikg::MultiArgs a{st.in(targets, sizeof(T) * 12 * T_),
                   T_,
                   st.in(seeds, sizeof(T) * nq * S),
                   S,
                   st.out(q_out, sizeof(T) * nq * T_),
                   (uint8_t*)st.out(converged, T_),
                   (int32_t*)st.out(iters, sizeof(int32_t) * T_),
                   st.out(err_out, sizeof(T) * 2 * T_),
                   (int32_t*)st.out(best_seed, sizeof(int32_t) * T_),
                   nq,
                   nullptr,
                   nullptr,
                   nullptr,
                   nullptr};
  if (st.rc) return st.rc;
  a.variant = params->variant;
  a.jit = model->jit_kernels<T>(device);
  a.ws_owner = &model->ws;
  if (dc) {
    a.collision = dc;
    a.n_geoms = model->col.k64.n_geoms;
  }
  // per-seed workspace, stream-ordered (capturable) allocation
  const int64_t n = T_ * S;
  const ikg::MultiLayout l(n, sizeof(T), nq);
  ikg::Workspace ws(&model->ws, s, "multistart");
  hipError_t e = ws.alloc(l);
  if (e != hipSuccess) return fail(IKG_ENOMEM, "multistart workspace allocation: %s", hipGetErrorString(e));
  a.ws_q = ws.at<void>(l.q);
  a.ws_err = ws.at<void>(l.err);
  a.ws_iters = ws.at<int32_t>(l.iters);
  a.ws_conv = ws.at<uint8_t>(l.conv);
  // the collision continuation's records, as solve_batch_t (same values for a
  // seed whatever call solves it)
  bool rec_used = false;
  ikg::Workspace rec(&model->ws, s, "rec");
  if (records_apply(model, params, a.collision != nullptr, a.jit != nullptr, nq) &&
      params->variant != IKG_VARIANT_QUAD) {
    a.rec_chunk = rec_chunk<T>(*params, T_, S);  // targets per launch (each with its S seeds)
    a.recs = offer_records<T>(rec, *params, a.rec_chunk * S, nq, &rec_used);
    if (!rec) a.rec_chunk = 0;
  }
  e = rec.finish(ikg::launch_multistart<T>(dm, kparams<T>(params), a, model->spec, s));
  const hipError_t e2 = ws.release();
  if (e != hipSuccess) return hip_fail(e, "ikg multistart kernel launch");
  if (e2 != hipSuccess) return hip_fail(e2, "multistart workspace free");
  return st.finish();
}

template <typename T>
int fk_t(ikg_model* model, int device, const void* q, int64_t B, void* hands, hipStream_t s, uint32_t flags) {
  const ikg::KModel<T>* dm = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc) return rc;
  Staging st(s, flags);
  const void* dq = st.in(q, sizeof(T) * model->desc.nq * B);
  void* dh = st.out(hands, sizeof(T) * 24 * B);
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_fk<T>(dm, dq, B, dh, s);
  if (e != hipSuccess) return hip_fail(e, "ikg fk kernel launch");
  return st.finish();
}

template <typename T>
int collision_t(ikg_model* model, int device, const void* q, const void* targets, int64_t B, uint8_t* out,
                hipStream_t s, uint32_t flags) {
  const ikg::KModel<T>* dm = nullptr;
  const ikg::KCollision<T>* dc = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc || (rc = model->col.get<T>(model->mu, device, &dc))) return rc;
  Staging st(s, flags);
  const void* dq = st.in(q, sizeof(T) * model->desc.nq * B);
  const void* dt = st.in(targets, sizeof(T) * 12 * B);
  uint8_t* dout = (uint8_t*)st.out(out, B);
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_collision<T>(dm, dc, dq, dt, B, dout, s);
  if (e != hipSuccess) return hip_fail(e, "ikg collision kernel launch");
  return st.finish();
}

template <typename T>
int log6_t(const void* M, int64_t B, void* out, hipStream_t s, uint32_t flags) {
  Staging st(s, flags);
  const void* dm = st.in(M, sizeof(T) * 12 * B);
  void* dout = st.out(out, sizeof(T) * 6 * B);
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_log6<T>(dm, B, dout, s);
  if (e != hipSuccess) return hip_fail(e, "ikg log6 kernel launch");
  return st.finish();
}

template <typename T>
int pair_state_t(ikg_model* model, int device, const void* targets, const void* q0, int64_t B, void* out) {
  const ikg::KModel<T>* dm = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc) return rc;
  Staging st(0, IKG_FLAG_HOST_POINTERS);
  const void* dt = st.in(targets, sizeof(T) * 12 * B);
  const void* dq = st.in(q0, sizeof(T) * model->desc.nq);
  void* dout = st.out(out, sizeof(T) * 62 * B);
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_pair_state<T>(dm, dt, dq, 0, B, dout, 0);
  if (e != hipSuccess) return hip_fail(e, "pair state kernel");
  return st.finish();
}

}  // namespace

extern "C" {

// Diagnostic (not in include/ikgrasp.h): per-lane iteration-0 state of the
// pair kernel, host pointers, q0 broadcast; out [B,2,31].
int ikg_debug_pair_state(const ikg_model* model, int device, int dtype, const void* targets, const void* q0,
                         int64_t B, void* out) {
  g_err[0] = 0;
  if (!model || B < 0) return fail(IKG_EINVAL, "bad arguments");
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  ikg_model* m = const_cast<ikg_model*>(model);
  return by_dtype(dtype, [&](auto t) { return pair_state_t<decltype(t)>(m, device, targets, q0, B, out); });
}

int ikg_log6_batch(int device, int dtype, const void* M, int64_t B, void* out, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > 0 && (!M || !out)) return fail(IKG_EINVAL, "M and out are required");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) { return log6_t<decltype(t)>(M, B, out, s, flags); });
}

const char* ikg_last_error(void) { return g_err; }

// Diagnostic (not in include/ikgrasp.h): scratch buffers held by captured
// graphs (live) and those whose graphs are gone (pending: reused by the next
// capture, freed by the model's next uncaptured solve or ikg_model_trim).
// tests/test_gpu_graph.py.
int ikg_debug_ws_count(const ikg_model* model, int64_t* live, int64_t* pending) {
  if (!model || !live || !pending) return fail(IKG_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> lock(model->ws.st->mu);
  *live = model->ws.st->live;
  *pending = (int64_t)model->ws.st->pending.size();
  return IKG_OK;
}

// Diagnostic (not in include/ikgrasp.h): bytes the model's scratch pools
// hold from the runtime (reserved) and hand out at the moment (used), summed
// over devices (hipMemPoolAttrReservedMemCurrent / UsedMemCurrent).
// tests/test_gpu_memory.py.
int ikg_debug_ws_pool(const ikg_model* model, int64_t* reserved, int64_t* used) {
  if (!model || !reserved || !used) return fail(IKG_EINVAL, "bad arguments");
  *reserved = *used = 0;
  for (auto& dp : ikg::ws_pools(const_cast<ikg::WsOwner*>(&model->ws), false)) {
    uint64_t r = 0, u = 0;
    if (hipMemPoolGetAttribute(dp.second, hipMemPoolAttrReservedMemCurrent, &r) != hipSuccess ||
        hipMemPoolGetAttribute(dp.second, hipMemPoolAttrUsedMemCurrent, &u) != hipSuccess)
      return fail(IKG_EHIP, "hipMemPoolGetAttribute failed");
    *reserved += (int64_t)r;
    *used += (int64_t)u;
  }
  return IKG_OK;
}

const char* ikg_version(void) { return "ikgrasp 0.1.0 (gfx950, pair kernel)"; }

void ikg_params_default(ikg_params* p) {
  if (!p) return;
  p->eps = 1e-3;       // config.py:22
  p->dt = 1e-2;        // inverse_geometry.py:54
  p->max_iters = 1000;  // inverse_geometry.py:53
  p->variant = IKG_VARIANT_AUTO;
  p->lambda = 0.0;      // np.linalg.pinv semantics
  p->problems_per_wave = 0;
  p->check_collision = 0;
}

int ikg_model_create(const ikg_model_desc* d, ikg_model** out) {
  g_err[0] = 0;
  if (!d || !out) return fail(IKG_EINVAL, "NULL argument");
  *out = nullptr;
  if (d->nq <= 0 || d->nq > IKG_MAX_NQ) return fail(IKG_EINVAL, "nq=%d outside [1,%d]", d->nq, IKG_MAX_NQ);
  for (int q = 0; q < d->nq; ++q) {
    if (d->axis[q] < 0 || d->axis[q] > 2) return fail(IKG_EINVAL, "joint %d: axis must be 0/1/2", q);
    if (d->parent[q] < -1 || d->parent[q] >= q)
      return fail(IKG_EINVAL, "joint %d: parent %d must precede it (Pinocchio order)", q, d->parent[q]);
    if (!(d->lower[q] <= d->upper[q])) return fail(IKG_EINVAL, "joint %d: lower > upper", q);
  }
  const int r = d->root_q;
  if (r < 0 || r >= d->nq || d->parent[r] != -1) return fail(IKG_EINVAL, "root_q must be a joint under the universe");
  bool used[IKG_MAX_NQ] = {};
  used[r] = true;
  for (int a = 0; a < 2; ++a) {
    int prev = r;
    for (int j = 0; j < IKG_ARM_DOF; ++j) {
      const int q = d->arm_q[a][j];
      if (q < 0 || q >= d->nq || used[q]) return fail(IKG_EINVAL, "arm %d joint %d: bad or repeated q index", a, j);
      if (d->parent[q] != prev) return fail(IKG_EINVAL, "arm %d joint %d: not a serial chain from the root", a, j);
      used[q] = true;
      prev = q;
    }
  }
  for (int j = 0; j < IKG_ARM_DOF; ++j)
    if (d->axis[d->arm_q[0][j]] != d->axis[d->arm_q[1][j]])
      return fail(IKG_EINVAL, "arm joint %d: left/right axes differ (unsupported)", j);
  ikg_model* m = new (std::nothrow) ikg_model();
  if (!m) return fail(IKG_ENOMEM, "out of host memory");
  m->desc = *d;
  ikg::build_kmodel<double>(*d, m->kin.k64);
  ikg::build_kmodel<float>(*d, m->kin.k32);
  m->spec = ikg::choose_spec(m->kin.k64);
  *out = m;
  return IKG_OK;
}

void ikg_model_destroy(ikg_model* m) {
  if (!m) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  m->kin.reset();
  m->col.reset();
  m->ine.reset();
  for (auto& v : m->jit)
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i]) {
        (void)hipSetDevice((int)i);
        ikg::jit_unload(*v[i]);
        delete v[i];
      }
  // scratch of captured graphs destroyed by now (a graph still alive keeps
  // its buffer: graphs must be destroyed before the model, whose tables they
  // also reference -- include/ikgrasp.h "Graphs")
  ikg::ws_drain(&m->ws);
  ikg::ws_pool_release(&m->ws);
  if (prev >= 0) (void)hipSetDevice(prev);
  delete m;
}

int ikg_model_trim(ikg_model* m) {
  g_err[0] = 0;
  if (!m) return fail(IKG_EINVAL, "model is NULL");
  int prev = -1;
  (void)hipGetDevice(&prev);
  ikg::ws_drain(&m->ws);  // buffers of destroyed graphs
  const hipError_t e = ikg::ws_pool_trim(&m->ws);
  if (prev >= 0) (void)hipSetDevice(prev);
  return e == hipSuccess ? IKG_OK : hip_fail(e, "ikg_model_trim");
}

int ikg_solve_batch(const ikg_model* model, int device, int dtype, const void* targets, const void* q0,
                    int64_t q0_stride, int64_t B, const ikg_params* params, void* q_out, uint8_t* converged,
                    int32_t* iters, void* err_out, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > 0 && (!targets || !q0 || !q_out)) return fail(IKG_EINVAL, "targets, q0 and q_out are required");
  if (q0_stride != 0 && q0_stride < model->desc.nq) return fail(IKG_EINVAL, "q0_stride must be 0 or >= nq");
  if (int rc = check_params(params)) return rc;
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  {
    const int ppw = params->problems_per_wave > 0 ? params->problems_per_wave : 32;
    if ((B + ppw - 1) / ppw > kMaxWaves) return fail(IKG_EINVAL, "B=%lld too large for one launch", (long long)B);
  }
  if (params->check_collision && B > kMaxWaves)
    return fail(IKG_EINVAL, "B=%lld too large for the collision launch (at most %lld)", (long long)B,
                (long long)kMaxWaves);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) {
    return solve_batch_t<decltype(t)>(m, device, targets, q0, q0_stride, B, params, q_out, converged, iters, err_out, s,
                                      flags);
  });
}

int ikg_solve_multistart(const ikg_model* model, int device, int dtype, const void* targets, int64_t T,
                         const void* seeds, int64_t S, const ikg_params* params, void* q_out, uint8_t* converged,
                         int32_t* iters, void* err_out, int32_t* best_seed, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (T < 0 || S <= 0) return fail(IKG_EINVAL, "need T >= 0 and S >= 1");
  if (S > (int64_t)1 << 24) return fail(IKG_EINVAL, "S=%lld seeds per target is too many", (long long)S);
  if (T > 0 && (!targets || !seeds || !q_out)) return fail(IKG_EINVAL, "targets, seeds and q_out are required");
  if (int rc = check_params(params)) return rc;
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  if (T > kMaxWaves || (T * S + 31) / 32 > kMaxWaves)
    return fail(IKG_EINVAL, "T=%lld x S=%lld too large for one launch", (long long)T, (long long)S);
  if (params->check_collision && T * S > kMaxWaves)
    return fail(IKG_EINVAL, "T*S=%lld too large for the collision launch (at most %lld)", (long long)(T * S),
                (long long)kMaxWaves);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (T == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) {
    return solve_multi_t<decltype(t)>(m, device, targets, T, seeds, S, params, q_out, converged, iters, err_out,
                                      best_seed, s, flags);
  });
}

int ikg_fk_batch(const ikg_model* model, int device, int dtype, const void* q, int64_t B, void* hands, void* stream,
                 uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > 0 && (!q || !hands)) return fail(IKG_EINVAL, "q and hands are required");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) { return fk_t<decltype(t)>(m, device, q, B, hands, s, flags); });
}

int ikg_model_set_collision(ikg_model* m, const ikg_collision_desc* d) {
  g_err[0] = 0;
  if (!m || !d) return fail(IKG_EINVAL, "NULL argument");
  if (d->n_geoms < 1 || d->n_geoms > IKG_MAX_GEOMS)
    return fail(IKG_EINVAL, "n_geoms=%d outside [1,%d]", d->n_geoms, IKG_MAX_GEOMS);
  if (d->n_pairs < 0 || d->n_pairs > IKG_MAX_PAIRS)
    return fail(IKG_EINVAL, "n_pairs=%d outside [0,%d]", d->n_pairs, IKG_MAX_PAIRS);
  if (d->target_geom < -1 || d->target_geom >= d->n_geoms) return fail(IKG_EINVAL, "target_geom out of range");
  for (int g = 0; g < d->n_geoms; ++g) {
    if (d->kind[g] < IKG_GEOM_SPHERE || d->kind[g] > IKG_GEOM_MESHBOX)
      return fail(IKG_EINVAL, "geometry %d: unknown kind %d", g, d->kind[g]);
    if (d->joint[g] < -1 || d->joint[g] >= m->desc.nq)
      return fail(IKG_EINVAL, "geometry %d: joint %d out of range", g, d->joint[g]);
    for (int i = 0; i < 3; ++i)
      if (!(d->dims[g][i] >= 0) || !std::isfinite(d->dims[g][i]))
        return fail(IKG_EINVAL, "geometry %d: dims must be finite and >= 0", g);
  }
  for (int k = 0; k < d->n_pairs; ++k) {
    const int a = d->pairs[k][0], b = d->pairs[k][1];
    if (a < 0 || b < 0 || a >= d->n_geoms || b >= d->n_geoms || a == b)
      return fail(IKG_EINVAL, "pair %d: bad geometry indices (%d, %d)", k, a, b);
  }
  std::lock_guard<std::mutex> lock(m->mu);
  m->col.reset();
  ikg::build_kcollision<double>(*d, m->col.k64);
  ikg::build_kcollision<float>(*d, m->col.k32);
  m->col.present = true;
  return IKG_OK;
}

int ikg_collision_batch(const ikg_model* model, int device, int dtype, const void* q, const void* targets, int64_t B,
                        uint8_t* in_collision, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > 0 && (!q || !targets || !in_collision)) return fail(IKG_EINVAL, "q, targets and in_collision are required");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  if (!model->col.present) return fail(IKG_EINVAL, "%s", model->col.missing);
  if (B > kMaxWaves) return fail(IKG_EINVAL, "B=%lld too large for one launch (at most %lld)", (long long)B, (long long)kMaxWaves);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) {
    return collision_t<decltype(t)>(m, device, q, targets, B, in_collision, s, flags);
  });
}

}  // extern "C"

// Small index arrays of the planner queries: host -> device each call.
template <typename T>
int distance_t(ikg_model* model, int device, const void* q, const void* targets, int64_t B, const int32_t* idx,
               int32_t n, void* out, hipStream_t s, uint32_t flags) {
  const ikg::KModel<T>* dm = nullptr;
  const ikg::KCollision<T>* dc = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc || (rc = model->col.get<T>(model->mu, device, &dc))) return rc;
  Staging st(s, flags);
  const int32_t* didx = (const int32_t*)st.upload(idx, sizeof(int32_t) * n);
  const void* dq = st.in(q, sizeof(T) * model->desc.nq * B);
  const void* dt = st.in(targets, sizeof(T) * 12 * B);
  void* dout = st.out(out, sizeof(T) * B);
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_distance<T>(dm, dc, dq, dt, B, didx, n, dout, s);
  if (e != hipSuccess) return hip_fail(e, "ikg distance kernel launch");
  return st.finish(true);  // the staged index array is freed on return
}

template <typename T>
int target_env_t(ikg_model* model, int device, const void* targets, int64_t B, const int32_t* geoms, int32_t n,
                 uint8_t* out, hipStream_t s, uint32_t flags) {
  const ikg::KCollision<T>* dc = nullptr;
  int rc = model->col.get<T>(model->mu, device, &dc);
  if (rc) return rc;
  Staging st(s, flags);
  const int32_t* dg = (const int32_t*)st.upload(geoms, sizeof(int32_t) * n);
  const void* dt = st.in(targets, sizeof(T) * 12 * B);
  uint8_t* dout = (uint8_t*)st.out(out, B);
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_target_env<T>(dc, dt, B, dg, n, dout, s);
  if (e != hipSuccess) return hip_fail(e, "ikg target/env kernel launch");
  return st.finish(true);  // the staged geometry list is freed on return
}

extern "C" {

int ikg_distance_batch(const ikg_model* model, int device, int dtype, const void* q, const void* targets,
                       int64_t B, const int32_t* pair_idx, int32_t n_pairs, void* dist, void* stream,
                       uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (n_pairs < 1 || !pair_idx) return fail(IKG_EINVAL, "pair_idx must list at least one pair");
  if (B > 0 && (!q || !targets || !dist)) return fail(IKG_EINVAL, "q, targets and dist are required");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  if (!model->col.present) return fail(IKG_EINVAL, "%s", model->col.missing);
  for (int32_t k = 0; k < n_pairs; ++k)
    if (pair_idx[k] < 0 || pair_idx[k] >= model->col.k64.n_pairs)
      return fail(IKG_EINVAL, "pair_idx[%d] = %d outside [0, %d)", k, pair_idx[k], model->col.k64.n_pairs);
  if (B > kMaxWaves) return fail(IKG_EINVAL, "B=%lld too large for one launch (at most %lld)", (long long)B, (long long)kMaxWaves);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) {
    return distance_t<decltype(t)>(m, device, q, targets, B, pair_idx, n_pairs, dist, s, flags);
  });
}

int ikg_target_env_batch(const ikg_model* model, int device, int dtype, const void* targets, int64_t B,
                         const int32_t* geoms, int32_t n_geoms, uint8_t* in_collision, void* stream,
                         uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (n_geoms < 1 || !geoms) return fail(IKG_EINVAL, "geoms must list at least one geometry");
  if (B > 0 && (!targets || !in_collision)) return fail(IKG_EINVAL, "targets and in_collision are required");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  if (!model->col.present) return fail(IKG_EINVAL, "%s", model->col.missing);
  for (int32_t k = 0; k < n_geoms; ++k)
    if (geoms[k] < 0 || geoms[k] >= model->col.k64.n_geoms || geoms[k] == model->col.k64.target_geom)
      return fail(IKG_EINVAL, "geoms[%d] = %d is not a scene geometry other than the target", k, geoms[k]);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) {
    return target_env_t<decltype(t)>(m, device, targets, B, geoms, n_geoms, in_collision, s, flags);
  });
}

}  // extern "C"

// ------------------------------------------------------------ controller kinematics
template <typename T>
int frame_kin_t(ikg_model* model, int device, const void* q, const void* v, const void* qd, const void* vd, int64_t B,
                int rf, const ikg_frame_kin_out& out, hipStream_t s, uint32_t flags) {
  const ikg::KModel<T>* dm = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc) return rc;
  const int nq = model->desc.nq;
  const size_t row = sizeof(T) * B, rows = row * nq;
  Staging st(s, flags);
  const bool des = out.err || out.derr;
  const void* dq = st.in(q, rows);
  const void* dv = st.in(v, rows);
  const void* dqd = des ? st.in(qd, rows) : nullptr;
  const void* dvd = des ? st.in(vd, rows) : nullptr;
  const ikg::FrameKinOut o{st.out(out.placement, 24 * row), st.out(out.velocity, 12 * row), st.out(out.J, 12 * rows),
                           st.out(out.dJ, 12 * rows),       st.out(out.dJv, 12 * row),      st.out(out.err, 12 * row),
                           st.out(out.derr, 12 * row)};
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_frame_kin<T>(dm, nq, model->spec, dq, dv, dqd, dvd, B, rf, o, s);
  if (e != hipSuccess) return hip_fail(e, "ikg frame kinematics kernel launch");
  return st.finish();
}

extern "C" {

int ikg_frame_kinematics_batch(const ikg_model* model, int device, int dtype, const void* q, const void* v,
                               const void* q_des, const void* v_des, int64_t B, int rf,
                               const ikg_frame_kin_out* out, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (!out) return fail(IKG_EINVAL, "out is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (rf < IKG_WORLD || rf > IKG_LOCAL_WORLD_ALIGNED) return fail(IKG_EINVAL, "rf %d unknown", rf);
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  if (B > 0 && !q) return fail(IKG_EINVAL, "q is required");
  if (B > 0 && (out->err || out->derr) && !q_des) return fail(IKG_EINVAL, "err/derr need q_des");
  if (B > (int64_t)1 << 40) return fail(IKG_EINVAL, "B too large");
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) {
    return frame_kin_t<decltype(t)>(m, device, q, v, q_des, v_des, B, rf, *out, s, flags);
  });
}

}  // extern "C"

// ------------------------------------------------------------ controller dynamics
template <typename T>
int dynamics_t(ikg_model* model, int device, const void* q, const void* v, int64_t B, const ikg_dynamics_out& out,
               hipStream_t s, uint32_t flags) {
  const ikg::KModel<T>* dm = nullptr;
  int rc = model->kin.get<T>(model->mu, device, &dm);
  if (rc) return rc;
  const ikg::KInertia<T>* di = nullptr;
  if ((rc = model->ine.get<T>(model->mu, device, &di))) return rc;
  const int nq = model->desc.nq;
  const size_t rows = sizeof(T) * nq * B;
  Staging st(s, flags);
  const void* dq = st.in(q, rows);
  const void* dv = st.in(v, rows);
  const ikg::DynOut o{st.out(out.M, rows * nq), st.out(out.nle, rows), st.out(out.g, rows)};
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_dynamics<T>(dm, di, nq, dq, dv, B, o, s);
  if (e != hipSuccess) return hip_fail(e, "ikg dynamics kernel launch");
  return st.finish();
}

extern "C" {

int ikg_model_set_inertia(ikg_model* m, const ikg_inertia_desc* d) {
  g_err[0] = 0;
  if (!m || !d) return fail(IKG_EINVAL, "NULL argument");
  const char* why = "";
  const int bad = ikg::check_inertia_desc(*d, m->desc.nq, &why);
  if (bad >= 0) return fail(IKG_EINVAL, "inertia of body %d: %s", bad, why);
  std::lock_guard<std::mutex> lock(m->mu);
  m->ine.reset();
  ikg::build_kinertia<double>(m->desc, *d, m->ine.k64);
  ikg::build_kinertia<float>(m->desc, *d, m->ine.k32);
  m->ine.present = true;
  return IKG_OK;
}

int ikg_dynamics_batch(const ikg_model* model, int device, int dtype, const void* q, const void* v, int64_t B,
                       const ikg_dynamics_out* out, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (!out) return fail(IKG_EINVAL, "out is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  if (B > 0 && !q) return fail(IKG_EINVAL, "q is required");
  if (B > (int64_t)1 << 40) return fail(IKG_EINVAL, "B too large");
  if (!model->ine.present) return fail(IKG_EINVAL, "%s", model->ine.missing);
  const int nq = model->desc.nq;  // (the device code is built with -ffinite-math-only)
  if (int rc = by_dtype(dtype, [&](auto t) {
        return check_finite_rows<decltype(t)>(flags, B, {{q, nq, "q"}, {v, nq, "v"}});
      }))
    return rc;
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) { return dynamics_t<decltype(t)>(m, device, q, v, B, *out, s, flags); });
}

}  // extern "C"

// ------------------------------------------------------------ controller torques
namespace {

// states per pass of ikg_control_torque_batch: its scratch (M, nle, J, dJ v, e,
// e' per state: 3.6 KB at nq = 15) stays at 240 MB whatever the batch
constexpr int64_t kCtlChunk = 65536;

// the gains, with the rollout's two time steps `dt` (null for the torque law alone)
int check_control_params(const ikg_control_params& c, const double* dt) {
  const double g[8] = {c.Kp, c.Kv, c.Kf, c.Kt, c.lambda_reg, c.qp_reg, dt ? dt[0] : 0.0, dt ? dt[1] : 0.0};
  int rc = check_finite<double>(g, dt ? 8 : 6, dt ? "gains / dt" : "gains");
  if (!rc) rc = check_finite<double>(c.fc_bias, 12, "fc_bias");
  if (rc) return rc;
  if (!(c.lambda_reg > 0) || !(c.qp_reg > 0))
    return fail(IKG_EINVAL, "lambda_reg and qp_reg must be > 0 (they make the factored matrices positive definite)");
  return IKG_OK;
}

// What every fp64 controller entry starts with: the scratch of destroyed graphs
// is released and the joint and inertia tables are on the device.
struct CtlTables {
  const ikg::KModel<double>* dm = nullptr;
  const ikg::KInertia<double>* di = nullptr;
};
int controller_tables(ikg_model* model, int device, hipStream_t s, CtlTables& t) {
  if (!ikg::stream_capturing(s)) ikg::ws_drain(&model->ws);
  if (int rc = model->kin.get<double>(model->mu, device, &t.dm)) return rc;
  return model->ine.get<double>(model->mu, device, &t.di);
}

// `bytes` of the model's stream-ordered scratch, poisoned, around body(ws, what):
// freed whatever the body returns; `what` names the launch that failed.
template <typename F>
int with_scratch(ikg_model* model, size_t bytes, hipStream_t s, const char* name, F&& body) {
  ikg::WsLayout l;
  l.add(bytes, ikg::WsLayout::kFloat, 1);
  ikg::Workspace ws(&model->ws, s, name);
  hipError_t e = ws.alloc(l);
  if (e != hipSuccess) return fail(IKG_ENOMEM, "%s scratch (%zu bytes): %s", name, bytes, hipGetErrorString(e));
  const char* what = "";
  e = body(ws.at<void>(0), what);
  const hipError_t ef = ws.release();
  if (e != hipSuccess) return hip_fail(e, what);
  if (ef != hipSuccess) return fail(IKG_EHIP, "%s scratch free: %s", name, hipGetErrorString(ef));
  return IKG_OK;
}

// pass(off, n) over the batch in chunks, until one fails
template <typename F>
hipError_t for_chunks(int64_t B, int64_t chunk, F&& pass) {
  hipError_t e = hipSuccess;
  for (int64_t off = 0; off < B && e == hipSuccess; off += chunk) e = pass(off, std::min(chunk, B - off));
  return e;
}

// state `off` of a [B, width] fp64 array; null (an absent array) stays null
const void* row_at(const void* p, size_t width, int64_t off) { return p ? (const double*)p + width * off : nullptr; }
void* row_at(void* p, size_t width, int64_t off) { return p ? (double*)p + width * off : nullptr; }

// The torque law's scratch for `chunk` states: M, J, nle, dJ v, e, e'
struct CtlScratch {
  double *M, *J, *nle, *dJv, *err, *derr, *end;
  static size_t per_state(int nq) { return (size_t)nq * nq + 12 * (size_t)nq + nq + 36; }
  CtlScratch(void* ws, int nq, int64_t chunk) {
    M = (double*)ws;
    J = M + (size_t)nq * nq * chunk;
    nle = J + 12 * (size_t)nq * chunk;
    dJv = nle + (size_t)nq * chunk;
    err = dJv + 12 * chunk;
    derr = err + 12 * chunk;
    end = derr + 12 * chunk;
  }
};

// frame kinematics, then dynamics, of n states into the scratch -> the input of the solve and step kernels
hipError_t torque_law_inputs(const ikg_model* model, const CtlTables& t, const CtlScratch& w, const void* q,
                             const void* v, const void* qd, const void* vd, int64_t n, hipStream_t s,
                             const char*& what, ikg::CtlIn& in) {
  const int nq = model->desc.nq;
  in = ikg::CtlIn{w.M, w.nle, w.J, w.dJv, w.err, w.derr};
  what = "ikg frame kinematics kernel launch";
  const hipError_t e =
      ikg::launch_frame_kin<double>(t.dm, nq, model->spec, q, v, qd, vd, n, IKG_LOCAL_WORLD_ALIGNED,
                                    ikg::FrameKinOut{nullptr, nullptr, w.J, nullptr, w.dJv, w.err, w.derr}, s);
  if (e != hipSuccess) return e;
  what = "ikg dynamics kernel launch";
  return ikg::launch_dynamics<double>(t.dm, t.di, nq, q, v, n, ikg::DynOut{w.M, w.nle, nullptr}, s);
}

int control_torque(ikg_model* model, int device, const void* q, const void* v, const void* qd, const void* vd,
                   int64_t B, const ikg_control_params& params, const ikg_control_out& out, hipStream_t s,
                   uint32_t flags) {
  using T = double;
  CtlTables t;
  if (int rc = controller_tables(model, device, s, t)) return rc;
  const int nq = model->desc.nq;
  const size_t rows = sizeof(T) * nq * B;
  Staging st(s, flags);
  const void *dq = st.in(q, rows), *dv = st.in(v, rows), *dqd = st.in(qd, rows), *dvd = st.in(vd, rows);
  const size_t sz[5] = {(size_t)nq, (size_t)nq, 12, 72, 12};  // per state
  void* o[5] = {out.tau, out.qdd, out.xdd, out.Lambda, out.fc};
  for (int i = 0; i < 5; ++i) o[i] = st.out(o[i], sizeof(T) * sz[i] * B);
  if (st.rc) return st.rc;
  const int64_t chunk = std::min(B, kCtlChunk);
  const ikg::KCtl<T> prm = ikg::make_kctl<T>(params);
  const int rc = with_scratch(
      model, sizeof(T) * CtlScratch::per_state(nq) * chunk, s, "controller", [&](void* ws, const char*& what) {
        const CtlScratch w(ws, nq, chunk);
        return for_chunks(B, chunk, [&](int64_t off, int64_t n) {
          ikg::CtlIn in;
          const hipError_t e = torque_law_inputs(model, t, w, row_at(dq, nq, off), row_at(dv, nq, off),
                                                 row_at(dqd, nq, off), row_at(dvd, nq, off), n, s, what, in);
          if (e != hipSuccess) return e;
          what = "ikg controller solve kernel launch";
          const ikg::CtlOut co{row_at(o[0], sz[0], off), row_at(o[1], sz[1], off), row_at(o[2], sz[2], off),
                               row_at(o[3], sz[3], off), row_at(o[4], sz[4], off)};
          return ikg::launch_control_solve(in, nq, n, prm, co, s);
        });
      });
  return rc ? rc : st.finish();
}

}  // namespace

extern "C" {

void ikg_control_params_default(ikg_control_params* p) {
  if (!p) return;
  p->Kp = 7000.0;                // control.py:248
  p->Kv = 2.0 * std::sqrt(p->Kp);  // :249
  p->Kf = 30.0;                  // :250
  p->Kt = 2.0 * std::sqrt(p->Kf);  // :251
  p->lambda_reg = 1e-6;          // :349
  p->qp_reg = 1e-6;              // :386
  for (int i = 0; i < 12; ++i) p->fc_bias[i] = 0.0;
  p->fc_bias[1] = -200.0;        // :375
  p->zero_tau_mask = (1u << 1) | (1u << 2);  // :404
}

int ikg_control_torque_batch(const ikg_model* model, int device, const void* q, const void* v, const void* q_des,
                             const void* v_des, int64_t B, const ikg_control_params* params,
                             const ikg_control_out* out, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (!out) return fail(IKG_EINVAL, "out is NULL");
  if (!params) return fail(IKG_EINVAL, "params is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > 0 && (!q || !q_des)) return fail(IKG_EINVAL, "q and q_des are required");
  if (B > (int64_t)1 << 40) return fail(IKG_EINVAL, "B too large");
  if (!model->ine.present) return fail(IKG_EINVAL, "%s", model->ine.missing);
  if (int rc = check_control_params(*params, nullptr)) return rc;
  const int nq = model->desc.nq;  // (the device code is built with -ffinite-math-only)
  if (int rc = check_finite_rows<double>(
          flags, B, {{q, nq, "q"}, {v, nq, "v"}, {q_des, nq, "q_des"}, {v_des, nq, "v_des"}}))
    return rc;
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  return control_torque(const_cast<ikg_model*>(model), device, q, v, q_des, v_des, B, *params, *out,
                        (hipStream_t)stream, flags);
}

}  // extern "C"

// ------------------------------------------------------------ forward dynamics, Bezier curves, closed-loop rollout
namespace {

int forward_dynamics(ikg_model* model, int device, const void* q, const void* v, const void* tau, int64_t B,
                     void* qdd, hipStream_t s, uint32_t flags) {
  using T = double;
  CtlTables t;
  if (int rc = controller_tables(model, device, s, t)) return rc;
  const int nq = model->desc.nq;
  const size_t rows = sizeof(T) * nq * B;
  Staging st(s, flags);
  const void *dq = st.in(q, rows), *dv = st.in(v, rows), *dtau = st.in(tau, rows);
  void* dout = st.out(qdd, rows);
  if (st.rc) return st.rc;
  const int64_t chunk = std::min(B, kCtlChunk);
  const int rc = with_scratch(  // nle
      model, sizeof(T) * nq * chunk, s, "forward dynamics", [&](void* wn, const char*& what) {
        return for_chunks(B, chunk, [&](int64_t off, int64_t n) {
          what = "ikg dynamics kernel launch";
          const hipError_t e = ikg::launch_dynamics<T>(t.dm, t.di, nq, row_at(dq, nq, off), row_at(dv, nq, off), n,
                                                       ikg::DynOut{nullptr, wn, nullptr}, s);
          if (e != hipSuccess) return e;
          what = "ikg forward dynamics kernel launch";
          return ikg::launch_forward_dynamics(t.dm, t.di, nq, row_at(dq, nq, off), wn, row_at(dtau, nq, off), n,
                                              row_at(dout, nq, off), s);
        });
      });
  return rc ? rc : st.finish();
}


int check_bezier(const ikg_bezier* c, int dim, const char* what) {
  if (!c || !c->points) return fail(IKG_EINVAL, "%s: curve or its points are NULL", what);
  if (c->n_points < 2) return fail(IKG_EINVAL, "%s: a curve needs at least 2 control points", what);
  if (c->n_points > ikg::kMaxBezier)
    return fail(IKG_EINVAL, "%s: %d control points (max %d)", what, c->n_points, ikg::kMaxBezier);
  if (!std::isfinite(c->t_min) || !std::isfinite(c->t_max) || !(c->t_max > c->t_min))
    return fail(IKG_EINVAL, "%s: t_max must be above t_min", what);
  if (!std::isfinite(c->mult)) return fail(IKG_EINVAL, "%s: mult is not finite", what);
  return check_finite<double>(c->points, (int64_t)c->n_points * dim, what);
}

// [P (n x dim)] [bc (n)] of one curve
void append_curve(std::vector<double>& tab, const ikg_bezier& c, int dim) {
  tab.insert(tab.end(), c.points, c.points + (size_t)c.n_points * dim);
  double bc[ikg::kMaxBezier];
  ikg::bezier_coeffs(c.n_points, bc);
  tab.insert(tab.end(), bc, bc + c.n_points);
}

// [bc (n)] of a curve whose control points stay with the caller (one curve per state)
void append_coeffs(std::vector<double>& tab, int n_points) {
  double bc[ikg::kMaxBezier];
  ikg::bezier_coeffs(n_points, bc);
  tab.insert(tab.end(), bc, bc + n_points);
}

// A rollout's curve: one for all states (ikg_bezier, host control points) or one
// per state (ikg_bezier_set, [B,n_points,nq] device or host per flag)
struct CurveArg {
  const double* shared;
  const void* per_state;
  int32_t n_points;
  double t_min, t_max, mult;
  explicit CurveArg(const ikg_bezier& c)
      : shared(c.points), per_state(nullptr), n_points(c.n_points), t_min(c.t_min), t_max(c.t_max), mult(c.mult) {}
  explicit CurveArg(const ikg_bezier_set& c)
      : shared(nullptr), per_state(c.points), n_points(c.n_points), t_min(c.t_min), t_max(c.t_max), mult(c.mult) {}
  ikg_bezier one() const { return ikg_bezier{shared, n_points, t_min, t_max, mult}; }
};

int control_rollout(ikg_model* model, int device, const void* q0, const void* v0, const void* t0, int64_t B,
                    const CurveArg& bq, const CurveArg& bv, const ikg_rollout_params& params,
                    const ikg_rollout_out& out, hipStream_t s, uint32_t flags) {
  using T = double;
  CtlTables t;
  if (int rc = controller_tables(model, device, s, t)) return rc;
  const int nq = model->desc.nq;
  const int64_t ticks = params.ticks, every = params.record_every;
  const int64_t R = every > 0 ? ticks / every : 0;
  const size_t sz[6] = {(size_t)nq, (size_t)nq, 1, (size_t)(R * nq), (size_t)(R * nq), (size_t)(R * nq)};  // per state
  void* o[6] = {out.q, out.v, out.t, R ? out.q_hist : nullptr, R ? out.v_hist : nullptr, R ? out.tau_hist : nullptr};
  Staging st(s, flags);
  const void* dq0 = st.in(q0, sizeof(T) * nq * B);
  const void* dv0 = st.in(v0, sizeof(T) * nq * B);
  const void* dt0 = st.in(t0, sizeof(T) * B);
  for (int i = 0; i < 6; ++i) o[i] = st.out(o[i], sizeof(T) * sz[i] * B);
  const bool per_state = bq.per_state != nullptr;
  const int64_t stride_q = per_state ? (int64_t)bq.n_points * nq : 0;
  const int64_t stride_v = per_state ? (int64_t)bv.n_points * nq : 0;
  const void* dpq = per_state ? st.in(bq.per_state, sizeof(T) * stride_q * B) : nullptr;
  const void* dpv = per_state ? st.in(bv.per_state, sizeof(T) * stride_v * B) : nullptr;
  if (st.rc) return st.rc;
  std::vector<double> tab;
  if (per_state) {
    append_coeffs(tab, bq.n_points);
    append_coeffs(tab, bv.n_points);
  } else {
    append_curve(tab, bq.one(), nq);
    append_curve(tab, bv.one(), nq);
  }
  // scratch: the torque law's, the desired state, the state rows the caller
  // did not ask for, and the curve table
  const int64_t chunk = std::min(B, kCtlChunk);
  const size_t per = CtlScratch::per_state(nq) + 2 * (size_t)nq + (o[0] ? 0 : nq) + (o[1] ? 0 : nq) + (o[2] ? 0 : 1);
  const ikg::KCtl<T> prm = ikg::make_kctl<T>(params.control);
  const int rc = with_scratch(
      model, sizeof(T) * (per * chunk + tab.size()), s, "rollout", [&](void* ws, const char*& what) {
        const CtlScratch w(ws, nq, chunk);
        T* wqd = w.end;
        T* wvd = wqd + (size_t)nq * chunk;
        T* next = wvd + (size_t)nq * chunk;
        T *sq = nullptr, *sv = nullptr, *stt = nullptr;
        if (!o[0]) sq = next, next += (size_t)nq * chunk;
        if (!o[1]) sv = next, next += (size_t)nq * chunk;
        if (!o[2]) stt = next, next += chunk;
        T* wtab = next;
        what = "rollout curve table upload";
        const hipError_t e = ikg::launch_table_write(wtab, tab.data(), tab.size(), s);
        if (e != hipSuccess) return e;
        return for_chunks(B, chunk, [&](int64_t off, int64_t n) {
          ikg::StepArgs a;
          a.q = o[0] ? row_at(o[0], sz[0], off) : sq;
          a.v = o[1] ? row_at(o[1], sz[1], off) : sv;
          a.t = o[2] ? row_at(o[2], sz[2], off) : stt;
          a.qdes = wqd;
          a.vdes = wvd;
          a.cv = ikg::RolloutCurves{wtab,
                                    bq.n_points,
                                    bv.n_points,
                                    bq.t_min,
                                    bq.t_max,
                                    bq.mult,
                                    bv.t_min,
                                    bv.t_max,
                                    bv.mult,
                                    (const T*)row_at(dpq, stride_q, off),  // curves chunk with their states
                                    (const T*)row_at(dpv, stride_v, off),
                                    stride_q,
                                    stride_v};
          a.dt_sim = params.dt_sim;
          a.dt_traj = params.dt_traj;
          a.q_hist = row_at(o[3], sz[3], off);
          a.v_hist = row_at(o[4], sz[4], off);
          a.tau_hist = row_at(o[5], sz[5], off);
          a.R = R;
          a.slot = -1;
          what = "ikg rollout init kernel launch";
          hipError_t e = ikg::launch_rollout_init(row_at(dq0, nq, off), row_at(dv0, nq, off), row_at(dt0, 1, off), nq,
                                                  n, a, s);
          for (int64_t k = 0; k < ticks && e == hipSuccess; ++k) {
            ikg::CtlIn in;
            e = torque_law_inputs(model, t, w, a.q, a.v, wqd, wvd, n, s, what, in);
            if (e != hipSuccess) break;
            what = "ikg control step kernel launch";
            a.slot = (R && (k + 1) % every == 0 && (k + 1) / every <= R) ? (k + 1) / every - 1 : -1;
            e = ikg::launch_control_step(in, nq, n, prm, a, s);
          }
          return e;
        });
      });
  return rc ? rc : st.finish();
}

// the arguments both rollout entries share, before their curves
int check_rollout_args(const ikg_model* model, const void* q0, int64_t B, const ikg_rollout_params* params,
                       const ikg_rollout_out* out) {
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (!out) return fail(IKG_EINVAL, "out is NULL");
  if (!params) return fail(IKG_EINVAL, "params is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > 0 && !q0) return fail(IKG_EINVAL, "q0 is required");
  if (B > (int64_t)1 << 40) return fail(IKG_EINVAL, "B too large");
  if (!model->ine.present) return fail(IKG_EINVAL, "%s", model->ine.missing);
  return IKG_OK;
}

int check_bezier_set(const ikg_bezier_set* c, int dim, int64_t B, uint32_t flags, const char* what) {
  if (!c || (B > 0 && !c->points)) return fail(IKG_EINVAL, "%s: curves or their points are NULL", what);
  const double one = 0.0;  // check_bezier's rules for the sizes and the range
  const ikg_bezier b{&one, c->n_points, c->t_min, c->t_max, c->mult};
  if (int rc = check_bezier(&b, 0, what)) return rc;
  return check_finite_rows<double>(flags, B, {{c->points, (int64_t)c->n_points * dim, what}});
}

// the rest of a rollout entry once its curves passed
int rollout_entry(const ikg_model* model, int device, const void* q0, const void* v0, const void* t0, int64_t B,
                  const CurveArg& bq, const CurveArg& bv, const ikg_rollout_params& params,
                  const ikg_rollout_out& out, void* stream, uint32_t flags) {
  const int nq = model->desc.nq;
  const double dt[2] = {params.dt_sim, params.dt_traj};
  int rc = check_control_params(params.control, dt);
  if (rc) return rc;
  if (params.ticks < 0 || params.record_every < 0) return fail(IKG_EINVAL, "ticks and record_every must be >= 0");
  if ((out.q_hist || out.v_hist || out.tau_hist) && params.record_every == 0)
    return fail(IKG_EINVAL, "a history output needs record_every > 0");
  // (the device code is built with -ffinite-math-only)
  if ((rc = check_finite_rows<double>(flags, B, {{q0, nq, "q0"}, {v0, nq, "v0"}, {t0, 1, "t0"}}))) return rc;
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  return control_rollout(const_cast<ikg_model*>(model), device, q0, v0, t0, B, bq, bv, params, out,
                         (hipStream_t)stream, flags);
}

}  // namespace

extern "C" {

int ikg_forward_dynamics_batch(const ikg_model* model, int device, const void* q, const void* v, const void* tau,
                               int64_t B, void* qdd, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > 0 && (!q || !tau || !qdd)) return fail(IKG_EINVAL, "q, tau and qdd are required");
  if (B > (int64_t)1 << 40) return fail(IKG_EINVAL, "B too large");
  if (!model->ine.present) return fail(IKG_EINVAL, "%s", model->ine.missing);
  const int nq = model->desc.nq;  // (the device code is built with -ffinite-math-only)
  if (int rc = check_finite_rows<double>(flags, B, {{q, nq, "q"}, {v, nq, "v"}, {tau, nq, "tau"}})) return rc;
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  return forward_dynamics(const_cast<ikg_model*>(model), device, q, v, tau, B, qdd, (hipStream_t)stream, flags);
}

int ikg_bezier_eval_batch(int device, const double* points, int32_t n_points, int32_t dim, double t_min, double t_max,
                          double mult, const void* times, int64_t K, void* out, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (dim < 1 || dim > IKG_MAX_NQ) return fail(IKG_EINVAL, "dim must be in [1, %d]", IKG_MAX_NQ);
  const ikg_bezier c{points, n_points, t_min, t_max, mult};
  int rc = check_bezier(&c, dim, "points");
  if (rc) return rc;
  if (K < 0) return fail(IKG_EINVAL, "K must be >= 0");
  if (K > 0 && (!times || !out)) return fail(IKG_EINVAL, "times and out are required");
  if (K > (int64_t)1 << 40) return fail(IKG_EINVAL, "K too large");
  if (flags & IKG_FLAG_HOST_POINTERS) {
    const double* t = (const double*)times;
    for (int64_t k = 0; k < K; ++k)
      if (!(t[k] >= t_min && t[k] <= t_max))
        return fail(IKG_EINVAL, "times[%lld] = %g is outside [%g, %g]", (long long)k, t[k], t_min, t_max);
  }
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (K == 0) return IKG_OK;
  hipStream_t s = (hipStream_t)stream;
  std::vector<double> tab;
  append_curve(tab, c, dim);
  Staging st(s, flags);
  double* dtab = (double*)st.alloc(sizeof(double) * tab.size());
  const void* dt = st.in(times, sizeof(double) * K);
  void* dout = st.out(out, sizeof(double) * K * dim);
  if (st.rc) return st.rc;
  hipError_t e = ikg::launch_table_write(dtab, tab.data(), tab.size(), s);
  if (e == hipSuccess)
    e = ikg::launch_bezier_eval(dtab, n_points, dim, t_min, t_max, mult, (const double*)dt, K, (double*)dout, s);
  if (e != hipSuccess) return hip_fail(e, "ikg bezier kernel launch");
  return st.finish(true);  // the table is freed on return
}

void ikg_rollout_params_default(ikg_rollout_params* p) {
  if (!p) return;
  ikg_control_params_default(&p->control);
  p->dt_sim = 1e-3;   // config.py:21
  p->dt_traj = 1e-2;  // control.py:449, :463: DT = 0.01 per 1 ms simulator tick
  p->ticks = 0;
  p->record_every = 0;
}

int ikg_control_rollout(const ikg_model* model, int device, const void* q0, const void* v0, const void* t0, int64_t B,
                        const ikg_bezier* q_curve, const ikg_bezier* v_curve, const ikg_rollout_params* params,
                        const ikg_rollout_out* out, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (int rc = check_rollout_args(model, q0, B, params, out)) return rc;
  const int nq = model->desc.nq;
  int rc = check_bezier(q_curve, nq, "q_curve");
  if (!rc) rc = check_bezier(v_curve, nq, "v_curve");
  if (rc) return rc;
  return rollout_entry(model, device, q0, v0, t0, B, CurveArg(*q_curve), CurveArg(*v_curve), *params, *out, stream,
                       flags);
}

int ikg_control_rollout_curves(const ikg_model* model, int device, const void* q0, const void* v0, const void* t0,
                               int64_t B, const ikg_bezier_set* q_curves, const ikg_bezier_set* v_curves,
                               const ikg_rollout_params* params, const ikg_rollout_out* out, void* stream,
                               uint32_t flags) {
  g_err[0] = 0;
  if (int rc = check_rollout_args(model, q0, B, params, out)) return rc;
  const int nq = model->desc.nq;
  int rc = check_bezier_set(q_curves, nq, B, flags, "q_curves");
  if (!rc) rc = check_bezier_set(v_curves, nq, B, flags, "v_curves");
  if (rc) return rc;
  return rollout_entry(model, device, q0, v0, t0, B, CurveArg(*q_curves), CurveArg(*v_curves), *params, *out, stream,
                       flags);
}

void ikg_fit_params_default(ikg_fit_params* p) {
  if (!p) return;
  p->degree = 20;  // control.py:85
  p->ridge = 0.0;
  p->total_time = 1.0;
}

int ikg_bezier_fit_batch(int device, const void* q0, const void* q1, const void* path_points, const int64_t* offsets,
                         int64_t B, int32_t dim, const ikg_fit_params* params, void* points, void* vpoints,
                         void* apoints, void* cost, int32_t* status, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!params) return fail(IKG_EINVAL, "params is NULL");
  if (dim < 1 || dim > IKG_MAX_NQ) return fail(IKG_EINVAL, "dim must be in [1, %d]", IKG_MAX_NQ);
  const int d = params->degree;
  if (d < ikg::kFitMinDegree || d > ikg::kFitMaxDegree)
    return fail(IKG_EINVAL, "degree must be in [%d, %d]", ikg::kFitMinDegree, ikg::kFitMaxDegree);
  if (!std::isfinite(params->total_time) || !(params->total_time > 0))
    return fail(IKG_EINVAL, "total_time must be > 0");
  if (!std::isfinite(params->ridge) || !(params->ridge >= 0)) return fail(IKG_EINVAL, "ridge must be >= 0 and finite");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  if (B > (int64_t)1 << 40) return fail(IKG_EINVAL, "B too large");
  if (B > 0 && (!q0 || !q1 || !path_points || !offsets || !points || !cost || !status))
    return fail(IKG_EINVAL, "q0, q1, path_points, offsets, points, cost and status are required");
  int64_t total = 0;
  if (flags & IKG_FLAG_HOST_POINTERS) {
    if (B > 0 && offsets[0] != 0) return fail(IKG_EINVAL, "offsets[0] must be 0");
    for (int64_t p = 0; p < B; ++p) {
      const int64_t n = offsets[p + 1] - offsets[p];
      if (n < 2 || n > ikg::kFitMaxN)
        return fail(IKG_EINVAL, "path %lld has %lld points (2 .. %d)", (long long)p, (long long)n, ikg::kFitMaxN);
      if (!ikg::fit_count_ok(n, d, params->ridge))
        return fail(IKG_EINVAL, "path %lld has %lld points: degree %d needs %d unless ridge > 0", (long long)p,
                    (long long)n, d, d - 3);
    }
    total = B > 0 ? offsets[B] : 0;
    if (int rc = check_finite_rows<double>(flags, B, {{q0, dim, "q0"}, {q1, dim, "q1"}})) return rc;
    if (int rc = check_finite<double>(path_points, total * dim, "path_points")) return rc;
  }
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  hipStream_t s = (hipStream_t)stream;
  Staging st(s, flags);
  ikg::FitArgs a;
  a.q0 = (const double*)st.in(q0, sizeof(double) * dim * B);
  a.q1 = (const double*)st.in(q1, sizeof(double) * dim * B);
  a.y = (const double*)st.in(path_points, sizeof(double) * dim * total);
  a.offsets = (const int64_t*)st.in(offsets, sizeof(int64_t) * (B + 1));
  a.dim = dim;
  a.degree = d;
  a.ridge = params->ridge;
  a.T = params->total_time;
  a.points = (double*)st.out(points, sizeof(double) * (d + 1) * dim * B);
  a.vpoints = (double*)st.out(vpoints, sizeof(double) * d * dim * B);
  a.apoints = (double*)st.out(apoints, sizeof(double) * (d - 1) * dim * B);
  a.cost = (double*)st.out(cost, sizeof(double) * B);
  a.status = (int32_t*)st.out(status, sizeof(int32_t) * B);
  if (st.rc) return st.rc;
  ikg::bezier_coeffs(d + 1, a.bc);
  const hipError_t e = ikg::launch_bezier_fit(a, B, s);
  if (e != hipSuccess) return hip_fail(e, "ikg bezier fit kernel launch");
  return st.finish();
}

}  // extern "C"

// ------------------------------------------------------------ RRT-Connect planner (ikg_planner.hpp)
extern "C" {

int ikg_se3_interpolate_batch(int device, const void* A, const void* B, const void* alpha, int64_t C, void* out,
                              void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (C < 0) return fail(IKG_EINVAL, "C must be >= 0");
  if (C > (int64_t)1 << 40) return fail(IKG_EINVAL, "C too large");
  if (C > 0 && (!A || !B || !alpha || !out)) return fail(IKG_EINVAL, "A, B, alpha and out are required");
  if (int rc = check_finite_rows<double>(flags, C, {{A, 12, "A"}, {B, 12, "B"}, {alpha, 1, "alpha"}})) return rc;
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (C == 0) return IKG_OK;
  hipStream_t s = (hipStream_t)stream;
  Staging st(s, flags);
  const double* dA = (const double*)st.in(A, sizeof(double) * 12 * C);
  const double* dB = (const double*)st.in(B, sizeof(double) * 12 * C);
  const double* da = (const double*)st.in(alpha, sizeof(double) * C);
  double* dout = (double*)st.out(out, sizeof(double) * 12 * C);
  if (st.rc) return st.rc;
  const hipError_t e = ikg::launch_se3_interpolate(dA, dB, da, C, dout, s);
  if (e != hipSuccess) return hip_fail(e, "ikg se3 interpolate kernel launch");
  return st.finish();
}

int ikg_nearest_batch(int device, const void* nodes, int64_t cap, const int32_t* counts, const void* queries,
                      int32_t nq, int64_t P, int32_t* index, void* dist, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (P < 0) return fail(IKG_EINVAL, "P must be >= 0");
  if (P > kMaxWaves) return fail(IKG_EINVAL, "P=%lld too large for one launch (at most %lld)", (long long)P, (long long)kMaxWaves);
  if (cap < 0 || cap > INT32_MAX) return fail(IKG_EINVAL, "cap must be in [0, 2^31)");
  if (nq < 1) return fail(IKG_EINVAL, "nq must be >= 1");
  if (P > 0 && (!counts || !queries || !index || !dist || (cap > 0 && !nodes)))
    return fail(IKG_EINVAL, "nodes, counts, queries, index and dist are required");
  if (flags & IKG_FLAG_HOST_POINTERS) {
    for (int64_t p = 0; p < P; ++p) {
      if (counts[p] < 0 || counts[p] > cap)
        return fail(IKG_EINVAL, "counts[%lld] = %d outside [0, cap = %lld]", (long long)p, counts[p], (long long)cap);
      if (int rc = check_finite<double>((const double*)nodes + p * cap * nq, (int64_t)counts[p] * nq, "nodes")) return rc;
    }
    if (int rc = check_finite<double>(queries, P * nq, "queries")) return rc;
  }
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (P == 0) return IKG_OK;
  hipStream_t s = (hipStream_t)stream;
  Staging st(s, flags);
  const double* dn = (const double*)st.in(nodes, sizeof(double) * P * cap * nq);
  const int32_t* dc = (const int32_t*)st.in(counts, sizeof(int32_t) * P);
  const double* dq = (const double*)st.in(queries, sizeof(double) * P * nq);
  int32_t* di = (int32_t*)st.out(index, sizeof(int32_t) * P);
  double* dd = (double*)st.out(dist, sizeof(double) * P);
  if (st.rc) return st.rc;
  const hipError_t e = ikg::launch_nearest(dn, cap, dc, dq, nq, P, di, dd, s);
  if (e != hipSuccess) return hip_fail(e, "ikg nearest kernel launch");
  return st.finish();
}

int ikg_project_paths(const ikg_model* model, int device, const void* q_curr, const void* cube_curr,
                      const void* cube_rand, int64_t C, double step_size, int32_t max_nodes, const int32_t* geoms,
                      int32_t n_geoms, const ikg_params* params, void* robot_path, void* cube_path, int32_t* n_nodes,
                      int32_t* status, void* stream, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (C < 0) return fail(IKG_EINVAL, "C must be >= 0");
  if (C > kMaxWaves) return fail(IKG_EINVAL, "C=%lld too large for one launch (at most %lld)", (long long)C, (long long)kMaxWaves);
  if (!(step_size > 0) || !std::isfinite(step_size)) return fail(IKG_EINVAL, "step_size must be > 0");
  if (max_nodes < 1) return fail(IKG_EINVAL, "max_nodes must be >= 1");
  if (n_geoms < 1 || n_geoms > IKG_MAX_GEOMS || !geoms) return fail(IKG_EINVAL, "geoms must list 1 .. %d geometries", IKG_MAX_GEOMS);
  if (int rc = check_params(params)) return rc;
  if (C > 0 && (!q_curr || !cube_curr || !cube_rand || !robot_path || !cube_path || !n_nodes || !status))
    return fail(IKG_EINVAL, "q_curr, cube_curr, cube_rand, robot_path, cube_path, n_nodes and status are required");
  if (!model->col.present) return fail(IKG_EINVAL, "%s", model->col.missing);
  if (model->col.k64.target_geom < 0) return fail(IKG_EINVAL, "the collision scene has no target geometry");
  ikg::ProjectArgs a{};
  a.geoms.n = n_geoms;
  for (int32_t k = 0; k < n_geoms; ++k) {
    if (geoms[k] < 0 || geoms[k] >= model->col.k64.n_geoms || geoms[k] == model->col.k64.target_geom)
      return fail(IKG_EINVAL, "geoms[%d] = %d is not a scene geometry other than the target", k, geoms[k]);
    a.geoms.g[k] = geoms[k];
  }
  const int nq = model->desc.nq;
  if (int rc = check_finite_rows<double>(flags, C, {{q_curr, nq, "q_curr"}, {cube_curr, 12, "cube_curr"}, {cube_rand, 12, "cube_rand"}}))
    return rc;
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (C == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  const ikg::KCollision<double>* dc = nullptr;
  if (int rc = m->col.get<double>(m->mu, device, &dc)) return rc;
  // steps to enqueue: every chain ends within max_nodes - 1 steps; a host-pointer
  // call knows the longest chain (projection_host_steps)
  int64_t n_steps = (int64_t)max_nodes - 1;
  if (flags & IKG_FLAG_HOST_POINTERS) {
    int64_t bad = 0;
    n_steps = ikg::projection_host_steps((const double*)cube_curr, (const double*)cube_rand, C, step_size, max_nodes, &bad);
    if (n_steps < 0) return fail(IKG_EINVAL, "chain %lld: |dt| / step_size is too large", (long long)bad);
  }
  Staging st(s, flags);
  a.q_curr = (const double*)st.in(q_curr, sizeof(double) * nq * C);
  a.cube_curr = (const double*)st.in(cube_curr, sizeof(double) * 12 * C);
  a.cube_rand = (const double*)st.in(cube_rand, sizeof(double) * 12 * C);
  a.C = C;
  a.nq = nq;
  a.max_nodes = max_nodes;
  a.step_size = step_size;
  a.robot_path = (double*)st.out(robot_path, sizeof(double) * nq * max_nodes * C);
  a.cube_path = (double*)st.out(cube_path, sizeof(double) * 12 * max_nodes * C);
  a.n_nodes = (int32_t*)st.out(n_nodes, sizeof(int32_t) * C);
  a.status = (int32_t*)st.out(status, sizeof(int32_t) * C);
  if (st.rc) return st.rc;
  const ikg::ProjectLayout l(C, nq);
  ikg::Workspace ws(&m->ws, s, "project");
  hipError_t e = ws.alloc(l);
  if (e != hipSuccess) return fail(IKG_ENOMEM, "projection workspace allocation: %s", hipGetErrorString(e));
  a.targets = ws.at<double>(l.targets);
  a.q0 = ws.at<double>(l.q0);
  double* q = ws.at<double>(l.q);
  uint8_t* conv = ws.at<uint8_t>(l.conv);
  a.q = q;
  a.conv = conv;
  a.steps = ws.at<int32_t>(l.aux);
  a.free_ = a.steps + C;
  if (st.host) {  // rows past a chain's end are copied back too: defined, zero
    e = hipMemsetAsync(a.robot_path, 0, sizeof(double) * nq * max_nodes * C, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.cube_path, 0, sizeof(double) * 12 * max_nodes * C, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(paths)");
  }
  // step 1's prepare also writes row 0, the step counts and the states
  for (int64_t step = 1; step <= std::max<int64_t>(n_steps, 1); ++step) {
    e = ikg::launch_project_prepare(dc, a, (int)step, s);
    if (e != hipSuccess) return hip_fail(e, "ikg projection prepare kernel launch");
    if (step > n_steps) break;  // max_nodes = 1: the chains are cut at their first row
    if (int rc = solve_batch_t<double>(m, device, a.targets, a.q0, nq, C, params, q, conv, ws.at<int32_t>(l.iters),
                                       ws.at<double>(l.err), s, 0))
      return rc;
    e = ikg::launch_project_commit(a, (int)step, s);
    if (e != hipSuccess) return hip_fail(e, "ikg projection commit kernel launch");
  }
  e = ws.release();
  if (e != hipSuccess) return hip_fail(e, "projection workspace free");
  return st.finish();
}

void ikg_trajcheck_params_default(ikg_trajcheck_params* p) {
  if (!p) return;
  p->samples = 151;  // 15 s at 0.1 s: the demo's total_time
  p->cube_mode = IKG_CUBE_CARRIED;
  p->samples_per_wave = 0;
}

int ikg_trajcheck_samples_per_wave(int64_t B, int32_t samples) {
  if (B < 1 || samples < 2) return 0;
  return ikg::trajcheck_samples_per_wave(B, samples, 0);
}

int ikg_trajectory_check_batch(const ikg_model* model, int device, const ikg_bezier_set* q_curves, int64_t B,
                               const void* cube_fixed, const int32_t* pair_idx, int32_t n_pairs,
                               const ikg_trajcheck_params* params, const ikg_trajcheck_out* out, void* stream,
                               uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (!params) return fail(IKG_EINVAL, "params is NULL");
  if (!out) return fail(IKG_EINVAL, "out is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  const int S = params->samples;
  if (S < 2) return fail(IKG_EINVAL, "samples must be >= 2");
  if (params->samples_per_wave < 0) return fail(IKG_EINVAL, "samples_per_wave must be >= 0");
  if (params->cube_mode != IKG_CUBE_CARRIED && params->cube_mode != IKG_CUBE_FIXED)
    return fail(IKG_EINVAL, "cube_mode %d unknown", params->cube_mode);
  if (params->cube_mode == IKG_CUBE_FIXED && B > 0 && !cube_fixed)
    return fail(IKG_EINVAL, "IKG_CUBE_FIXED needs cube_fixed");
  if (n_pairs < 0 || (n_pairs > 0 && !pair_idx)) return fail(IKG_EINVAL, "pair_idx must hold n_pairs >= 0 entries");
  if (!model->col.present) return fail(IKG_EINVAL, "%s", model->col.missing);
  if (model->col.k64.target_geom < 0) return fail(IKG_EINVAL, "the collision scene has no target geometry");
  for (int32_t k = 0; k < n_pairs; ++k)
    if (pair_idx[k] < 0 || pair_idx[k] >= model->col.k64.n_pairs)
      return fail(IKG_EINVAL, "pair_idx[%d] = %d outside [0, %d)", k, pair_idx[k], model->col.k64.n_pairs);
  const int nq = model->desc.nq;
  if (int rc = check_bezier_set(q_curves, nq, B, flags, "q_curves")) return rc;
  if (params->cube_mode == IKG_CUBE_FIXED)
    if (int rc = check_finite_rows<double>(flags, B, {{cube_fixed, 12, "cube_fixed"}})) return rc;
  const int spw = ikg::trajcheck_samples_per_wave(B > 0 ? B : 1, S, params->samples_per_wave);
  const int chunks = (S + spw - 1) / spw;
  if (B * chunks > kMaxWaves || B * (int64_t)S > (int64_t)1 << 40)
    return fail(IKG_EINVAL, "B=%lld with %d samples is too large for one launch", (long long)B, S);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  if (ikg::stream_capturing(s)) return fail(IKG_EINVAL, "ikg_trajectory_check_batch is not capturable");
  ikg::ws_drain(&m->ws);
  const ikg::KModel<double>* dm = nullptr;
  const ikg::KCollision<double>* dc = nullptr;
  int rc = m->kin.get<double>(m->mu, device, &dm);
  if (rc || (rc = m->col.get<double>(m->mu, device, &dc))) return rc;
  const bool want_clearance = n_pairs > 0 && (out->min_clearance || out->arg_clearance || out->clearance);
  Staging st(s, flags);
  ikg::TrajCheckArgs a{};
  a.points = (const double*)st.in(q_curves->points, sizeof(double) * q_curves->n_points * nq * B);
  a.n_points = q_curves->n_points;
  a.t_min = q_curves->t_min;
  a.t_max = q_curves->t_max;
  a.mult = q_curves->mult;
  a.S = S;
  a.spw = spw;
  a.chunks = chunks;
  a.cube_mode = params->cube_mode;
  a.cube_fixed = a.cube_mode == IKG_CUBE_FIXED ? (const double*)st.in(cube_fixed, sizeof(double) * 12 * B) : nullptr;
  a.n_idx = want_clearance ? n_pairs : 0;
  a.pair_idx = want_clearance ? (const int32_t*)st.upload(pair_idx, sizeof(int32_t) * n_pairs) : nullptr;
  const size_t rows = (size_t)B * S;
  a.collision = (uint8_t*)st.out(out->collision, rows);
  a.clearance = (double*)st.out(out->clearance, sizeof(double) * rows);
  a.grasp = (double*)st.out(out->grasp, sizeof(double) * rows);
  a.limit = (double*)st.out(out->limit, sizeof(double) * rows);
  a.cube = (double*)st.out(out->cube, sizeof(double) * 12 * rows);
  ikg::TrajFoldOut o{};
  o.first_collision = (int32_t*)st.out(out->first_collision, sizeof(int32_t) * B);
  o.first_pair = (int32_t*)st.out(out->first_pair, sizeof(int32_t) * B);
  o.n_collision = (int32_t*)st.out(out->n_collision, sizeof(int32_t) * B);
  o.min_clearance = (double*)st.out(out->min_clearance, sizeof(double) * B);
  o.arg_clearance = (int32_t*)st.out(out->arg_clearance, sizeof(int32_t) * B);
  o.max_grasp = (double*)st.out(out->max_grasp, sizeof(double) * B);
  o.arg_grasp = (int32_t*)st.out(out->arg_grasp, sizeof(int32_t) * B);
  o.max_limit = (double*)st.out(out->max_limit, sizeof(double) * B);
  o.arg_limit = (int32_t*)st.out(out->arg_limit, sizeof(int32_t) * B);
  if (st.rc) return st.rc;
  // scratch: the binomial factors, then one partial per wave
  double bc[ikg::kMaxBezier] = {};
  ikg::bezier_coeffs(a.n_points, bc);
  const size_t bc_bytes = sizeof(double) * ikg::kMaxBezier;
  rc = with_scratch(m, bc_bytes + sizeof(ikg::TrajPartial) * (size_t)B * chunks, s, "trajectory check",
                    [&](void* ws, const char*& what) {
                      what = "trajectory check table upload";
                      const hipError_t e = ikg::launch_table_write((double*)ws, bc, ikg::kMaxBezier, s);
                      if (e != hipSuccess) return e;
                      a.bc = (const double*)ws;
                      a.part = (ikg::TrajPartial*)((char*)ws + bc_bytes);
                      what = "ikg trajectory check kernel launch";
                      return ikg::launch_trajcheck(dm, dc, a, B, o, s);
                    });
  return rc ? rc : st.finish(true);  // the staged pair list is freed on return
}

void ikg_trajdyn_params_default(ikg_trajdyn_params* p) {
  if (!p) return;
  p->samples = 151;  // the trajectory check's
  p->samples_per_wave = 0;
  for (int j = 0; j < IKG_MAX_NQ; ++j) p->velocity_limit[j] = p->effort_limit[j] = IKG_NO_LIMIT;
}

int ikg_trajectory_dynamics_batch(const ikg_model* model, int device, const ikg_bezier_set* q_curves, int64_t B,
                                  const ikg_trajdyn_params* params, const ikg_trajdyn_out* out, void* stream,
                                  uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (!params) return fail(IKG_EINVAL, "params is NULL");
  if (!out) return fail(IKG_EINVAL, "out is NULL");
  if (B < 0) return fail(IKG_EINVAL, "B must be >= 0");
  const int S = params->samples;
  if (S < 2) return fail(IKG_EINVAL, "samples must be >= 2");
  if (params->samples_per_wave < 0) return fail(IKG_EINVAL, "samples_per_wave must be >= 0");
  if (!model->ine.present) return fail(IKG_EINVAL, "%s", model->ine.missing);
  const int nq = model->desc.nq;
  for (int j = 0; j < nq; ++j) {  // (!(x > 0) refuses a NaN; an infinite limit is written IKG_NO_LIMIT)
    if (!(params->velocity_limit[j] > 0) || !std::isfinite(params->velocity_limit[j]))
      return fail(IKG_EINVAL, "velocity_limit[%d] must be > 0 and finite (IKG_NO_LIMIT = unlimited)", j);
    if (!(params->effort_limit[j] > 0) || !std::isfinite(params->effort_limit[j]))
      return fail(IKG_EINVAL, "effort_limit[%d] must be > 0 and finite (IKG_NO_LIMIT = unlimited)", j);
  }
  if (q_curves && q_curves->n_points < ikg::kTrajDynMinPoints)
    return fail(IKG_EINVAL, "q_curves: %d control points, the acceleration curve needs at least %d",
                q_curves->n_points, ikg::kTrajDynMinPoints);
  if (int rc = check_bezier_set(q_curves, nq, B, flags, "q_curves")) return rc;
  const int spw = ikg::trajdyn_samples_per_wave(B > 0 ? B : 1, S, params->samples_per_wave, nq <= 16 ? 4 : 2);
  const int chunks = (S + spw - 1) / spw;
  if (B * chunks > kMaxWaves || B * (int64_t)S > (int64_t)1 << 40)
    return fail(IKG_EINVAL, "B=%lld with %d samples is too large for one launch", (long long)B, S);
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  if (B == 0) return IKG_OK;
  ikg_model* m = const_cast<ikg_model*>(model);
  hipStream_t s = (hipStream_t)stream;
  if (ikg::stream_capturing(s)) return fail(IKG_EINVAL, "ikg_trajectory_dynamics_batch is not capturable");
  CtlTables t;
  if (int rc = controller_tables(m, device, s, t)) return rc;
  Staging st(s, flags);
  ikg::TrajDynArgs a{};
  a.points = (const double*)st.in(q_curves->points, sizeof(double) * q_curves->n_points * nq * B);
  a.n_points = q_curves->n_points;
  a.t_min = q_curves->t_min;
  a.t_max = q_curves->t_max;
  a.mult = q_curves->mult;
  ikg::trajdyn_curve_setup(a);
  a.S = S;
  a.spw = spw;
  a.chunks = chunks;
  for (int j = 0; j < ikg::kMaxNq; ++j) {
    a.vlim[j] = j < nq ? params->velocity_limit[j] : IKG_NO_LIMIT;
    a.elim[j] = j < nq ? params->effort_limit[j] : IKG_NO_LIMIT;
  }
  const size_t rows = (size_t)B * S * nq;
  a.tau = (double*)st.out(out->tau, sizeof(double) * rows);
  a.g = (double*)st.out(out->g, sizeof(double) * rows);
  ikg::TrajDynFoldOut o{};
  o.speed_scale = (double*)st.out(out->speed_scale, sizeof(double) * B);
  o.arg_speed = (int32_t*)st.out(out->arg_speed, sizeof(int32_t) * 2 * B);
  o.torque_use = (double*)st.out(out->torque_use, sizeof(double) * B);
  o.arg_torque_use = (int32_t*)st.out(out->arg_torque_use, sizeof(int32_t) * 2 * B);
  o.static_use = (double*)st.out(out->static_use, sizeof(double) * B);
  o.arg_static = (int32_t*)st.out(out->arg_static, sizeof(int32_t) * 2 * B);
  o.n_static = (int32_t*)st.out(out->n_static, sizeof(int32_t) * B);
  o.torque_scale = (double*)st.out(out->torque_scale, sizeof(double) * B);
  o.arg_torque_scale = (int32_t*)st.out(out->arg_torque_scale, sizeof(int32_t) * 2 * B);
  if (st.rc) return st.rc;
  const int rc = with_scratch(m, sizeof(ikg::TrajDynPartial) * (size_t)B * chunks, s, "trajectory dynamics",
                              [&](void* ws, const char*& what) {
                                a.part = (ikg::TrajDynPartial*)ws;
                                what = "ikg trajectory dynamics kernel launch";
                                return ikg::launch_trajdyn(t.dm, t.di, nq, a, B, o, s);
                              });
  return rc ? rc : st.finish();
}

}  // extern "C"

// ------------------------------------------------------------ model-specialised kernels
namespace {

// Compile (once per model and dtype) the pair kernels against this model's
// tables; the caller holds m->mu.
int jit_code_locked(ikg_model* m, int dtype) {
  std::vector<char>& code = m->jit_code[dtype == IKG_F64 ? 0 : 1];
  if (!code.empty()) return IKG_OK;
  const std::string src = dtype == IKG_F64 ? ikg::jit_source(m->kin.k64) : ikg::jit_source(m->kin.k32);
  const std::string err = ikg::jit_compile(src, code);
  if (!err.empty()) {
    code.clear();
    return fail(IKG_EHIP, "model specialisation: %s", err.c_str());
  }
  return IKG_OK;
}

}  // namespace

extern "C" {

int ikg_model_specialize(ikg_model* model, int device, int dtype, uint32_t flags) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  if (flags & ~IKG_SPECIALIZE_IF_GENERIC) return fail(IKG_EINVAL, "flags must be 0 or IKG_SPECIALIZE_IF_GENERIC");
  if ((flags & IKG_SPECIALIZE_IF_GENERIC) && model->spec == ikg::kSpecNextage) return IKG_OK;
  DeviceGuard g(device);
  if (g.rc) return g.rc;
  std::lock_guard<std::mutex> lock(model->mu);
  auto& slot = model->jit[dtype == IKG_F64 ? 0 : 1];
  if ((int)slot.size() > device && slot[device]) return IKG_OK;
  if (int rc = jit_code_locked(model, dtype)) return rc;
  ikg::JitKernels* k = new (std::nothrow) ikg::JitKernels();
  if (!k) return fail(IKG_ENOMEM, "out of host memory");
  const hipError_t e = ikg::jit_load(model->jit_code[dtype == IKG_F64 ? 0 : 1], *k);
  if (e != hipSuccess) {
    delete k;
    return hip_fail(e, "hipModuleLoadData(specialised kernels)");
  }
  if ((int)slot.size() <= device) slot.resize(device + 1, nullptr);
  slot[device] = k;
  return IKG_OK;
}

int ikg_model_is_specialized(const ikg_model* model, int device, int dtype) {
  if (!model || device < 0 || (dtype != IKG_F64 && dtype != IKG_F32)) return 0;
  ikg_model* m = const_cast<ikg_model*>(model);
  return dtype == IKG_F64 ? m->jit_kernels<double>(device) != nullptr : m->jit_kernels<float>(device) != nullptr;
}

// Diagnostic (not in include/ikgrasp.h; no GPU needed): run the specialising
// compile and report the code object's size; with `path`, also write the code
// object there (llvm-objdump -d for the ISA).
int ikg_debug_jit_compile(const ikg_model* model, int dtype, const char* path, size_t* code_size) {
  g_err[0] = 0;
  if (!model) return fail(IKG_EINVAL, "model is NULL");
  if (dtype != IKG_F64 && dtype != IKG_F32) return fail(IKG_EINVAL, "dtype %d unknown", dtype);
  ikg_model* m = const_cast<ikg_model*>(model);
  std::lock_guard<std::mutex> lock(m->mu);
  if (int rc = jit_code_locked(m, dtype)) return rc;
  const std::vector<char>& code = m->jit_code[dtype == IKG_F64 ? 0 : 1];
  if (code_size) *code_size = code.size();
  if (path) {
    FILE* f = fopen(path, "wb");
    if (!f) return fail(IKG_EINVAL, "cannot open %s", path);
    const size_t n = fwrite(code.data(), 1, code.size(), f);
    fclose(f);
    if (n != code.size()) return fail(IKG_EINVAL, "short write to %s", path);
  }
  return IKG_OK;
}

}  // extern "C"
