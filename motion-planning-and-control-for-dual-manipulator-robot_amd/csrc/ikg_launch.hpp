// Host-side launcher declarations shared by ikg_kernels.hip and ikg_capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "ikg_collision.hpp"
#include "ikg_device.hpp"
#include "ikg_dynamics.hpp"
#include "ikg_solve.hpp"
#include "ikg_ws_layout.hpp"

namespace ikg {

struct JitKernels;  // ikg_jit.hpp

// Runtime knobs.  env_int reads the environment afresh at every call.  A knob
// read once per process says so where it is read (`static const ... =
// env_int(...)`); every other knob is read per launch, so one process (the
// tests) can flip it between solves.
inline long long env_int(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e ? atoll(e) : dflt;
}
inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt) != 0; }

// Workspaces of captured solves.  Outside a stream capture a
// solve's scratch is stream-ordered: hipMallocAsync / hipFreeAsync.  Inside a
// capture those calls become graph memory nodes, and a 164 MB record buffer
// taken that way read back as zeros in a later replay after a process had
// used the default pool heavily (tests/test_gpu_graph.py with
// IKG_TRAJ_REC=1; the same buffer from hipMalloc passed every replay).  So a
// captured solve takes its scratch from hipMalloc (relaxed capture mode for
// the call) and hands it to the capturing graph as a user object
// (hipGraphRetainUserObject): the buffer lives exactly as long as the graph
// and its executable instantiations.  The user object's destructor may not
// call HIP, so it only queues the buffer on the model's pending list.  A
// later capture takes a pending buffer that is large enough instead of
// allocating (no HIP call), so a workload that recaptures every cycle and
// never solves uncaptured holds a bounded number of buffers; the rest are
// freed by the model's next uncaptured call, ikg_model_trim or
// ikg_model_destroy.  Every instantiation of one captured graph shares its
// scratch, so two of them must not run at the same time (include/ikgrasp.h,
// "Graphs").
struct WsBuf {
  int dev;
  void* p;
  size_t bytes;
  // recorded by the captured work at the buffer's last use (a node of the
  // graph): a later capture reuses the buffer only once it has completed, so
  // a launch of the destroyed graph still in flight keeps its scratch (ADVICE
  // r5: a user object may be released before its exec's last launch ends).
  hipEvent_t done = nullptr;
  bool reuse = true;  // false: the record could not be captured -- never reused
};

struct WsState {
  static constexpr int kDevs = 64;
  std::mutex mu;
  std::vector<WsBuf> pending;     // buffers whose graphs are gone
  std::vector<WsBuf> held;        // buffers of graphs still alive (their completion events)
  int64_t live = 0;               // buffers held by graphs
  hipMemPool_t pool[kDevs] = {};  // the model's scratch pools (ws_pool), per device
};

struct WsOwner {
  std::shared_ptr<WsState> st = std::make_shared<WsState>();
};

struct GraphScratch {  // one captured buffer, owned by its graph's user object
  std::shared_ptr<WsState> st;
  WsBuf b;
};

inline void graph_scratch_release(void* arg) {  // user-object destructor: no HIP calls here
  GraphScratch* g = static_cast<GraphScratch*>(arg);
  {
    std::lock_guard<std::mutex> lock(g->st->mu);
    WsBuf b = g->b;
    for (size_t i = 0; i < g->st->held.size(); ++i)
      if (g->st->held[i].p == b.p) {
        b.done = g->st->held[i].done;
        b.reuse = g->st->held[i].reuse;
        g->st->held.erase(g->st->held.begin() + i);
        break;
      }
    g->st->pending.push_back(b);
    --g->st->live;
  }
  delete g;
}

inline bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive;
}

// Free the buffers of graphs destroyed since the last call (never while the
// calling thread's stream is capturing: hipFree is not a capturable call).
inline void ws_drain(WsOwner* owner) {
  if (!owner) return;
  std::vector<WsBuf> v;
  {
    std::lock_guard<std::mutex> lock(owner->st->mu);
    v.swap(owner->st->pending);
  }
  if (v.empty()) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (auto& b : v) {
    (void)hipSetDevice(b.dev);
    (void)hipFree(b.p);  // synchronises: every launch that used it has ended
    if (b.done) (void)hipEventDestroy(b.done);
  }
  if (prev >= 0) (void)hipSetDevice(prev);
}

// The smallest pending buffer on `dev` of at least `bytes` whose last use has
// completed (its event, queried outside capture semantics), taken off the
// list for a capture to reuse, or null.
inline void* ws_take_pending(WsState& st, int dev, size_t bytes, size_t* got, hipEvent_t* done) {
  std::lock_guard<std::mutex> lock(st.mu);
  int best = -1;
  for (int i = 0; i < (int)st.pending.size(); ++i) {
    const WsBuf& b = st.pending[i];
    if (b.dev != dev || b.bytes < bytes || (best >= 0 && b.bytes >= st.pending[best].bytes) || !b.done || !b.reuse)
      continue;
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    const hipError_t q = hipEventQuery(b.done);
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (q == hipSuccess) best = i;
    else if (q != hipErrorNotReady) (void)hipGetLastError();
  }
  if (best < 0) return nullptr;
  const WsBuf b = st.pending[best];
  st.pending.erase(st.pending.begin() + best);
  *got = b.bytes;
  *done = b.done;
  return b.p;
}

// How much freed scratch a model's pool keeps mapped across synchronisations
// (its release threshold): 1.25 GiB by default -- a C2 collision solve's
// records (656 MB) and every record-free solve's scratch stay mapped for the
// next solve; anything above goes back to the driver at the next
// synchronisation, so an idle model holds at most 1.25 GiB per device.  A
// larger collision solve maps its records afresh each time: C3 fp32 + collision
// (5.2 GB) 1.82 -> 1.93 ms, the C4 share and C5 + collision within their spread
// (profiles/r06/records/; round 5 kept 6.5 GiB).
// IKG_WS_KEEP_MB overrides (0 = keep nothing, as the device's default pool).
inline uint64_t ws_keep_bytes() {
  static const uint64_t v = (uint64_t)env_int("IKG_WS_KEEP_MB", 1280) << 20;
  return v;
}

// The model's stream-ordered scratch pool, one per device it solves on, which
// keeps what a solve frees (up to ws_keep_bytes) for the next solve instead of
// returning it to the driver at every synchronisation, as the device's default
// pool does (threshold 0): a collision solve's record buffer (656 MB at C2)
// was otherwise mapped afresh on every call (1-1.5% of a collision solve).
// The pools are the model's: ikg_model_trim returns their unused memory,
// ikg_model_destroy destroys them (ws_pool_release).  IKG_WS_POOL=0: the
// device's default pool (A/B).
inline hipMemPool_t ws_pool(WsOwner* owner) {
  static const bool on = env_flag("IKG_WS_POOL", true);
  if (!on || !owner) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= WsState::kDevs) return nullptr;
  WsState& st = *owner->st;
  std::lock_guard<std::mutex> lock(st.mu);
  if (!st.pool[dev]) {
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    uint64_t keep = ws_keep_bytes();
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    st.pool[dev] = pool;
  }
  return st.pool[dev];
}

// Every device the model has a pool on, with the pool handles copied out
// under the lock (`take`: and cleared, for ws_pool_release).  The callers
// synchronise and call into HIP outside the lock: graph_scratch_release takes
// the same mutex and may run on a runtime thread while a device synchronises.
inline std::vector<std::pair<int, hipMemPool_t>> ws_pools(WsOwner* owner, bool take) {
  std::vector<std::pair<int, hipMemPool_t>> v;
  if (!owner) return v;
  WsState& st = *owner->st;
  std::lock_guard<std::mutex> lock(st.mu);
  for (int d = 0; d < WsState::kDevs; ++d)
    if (st.pool[d]) {
      v.emplace_back(d, st.pool[d]);
      if (take) st.pool[d] = nullptr;
    }
  return v;
}

// Destroy the model's pools (ikg_model_destroy): each device is synchronised
// first, so the stream-ordered frees of its last solves have run.
inline void ws_pool_release(WsOwner* owner) {
  for (auto& dp : ws_pools(owner, true)) {
    (void)hipSetDevice(dp.first);
    (void)hipDeviceSynchronize();
    (void)hipMemPoolDestroy(dp.second);
  }
}

// Return the pools' unused memory to the driver (ikg_model_trim): each device
// is synchronised, then its pool trimmed to nothing kept; the pool stays
// usable.
inline hipError_t ws_pool_trim(WsOwner* owner) {
  hipError_t rc = hipSuccess;
  for (auto& dp : ws_pools(owner, false)) {
    (void)hipSetDevice(dp.first);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemPoolTrimTo(dp.second, 0);
    if (e != hipSuccess && rc == hipSuccess) rc = e;
  }
  return rc;
}

inline hipError_t ws_alloc(WsOwner* owner, void** p, size_t bytes, hipStream_t s) {
  *p = nullptr;
  if (!owner || !stream_capturing(s)) {
    if (hipMemPool_t pool = ws_pool(owner)) return hipMallocFromPoolAsync(p, bytes, pool, s);
    return hipMallocAsync(p, bytes, s);
  }
  hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamGetCaptureInfo_v2(s, &cst, nullptr, &graph, nullptr, nullptr);
  if (e != hipSuccess || !graph) return e != hipSuccess ? e : hipErrorStreamCaptureInvalidated;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const size_t want = bytes ? bytes : 1;
  size_t got = want;
  hipEvent_t done = nullptr;
  *p = ws_take_pending(*owner->st, dev, want, &got, &done);  // a destroyed graph's buffer, its last launch ended
  if (!*p) {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    e = hipMalloc(p, want);
    if (e == hipSuccess && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      done = nullptr;
    }
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (e != hipSuccess) {
      *p = nullptr;
      return e;
    }
  }
  {
    std::lock_guard<std::mutex> lock(owner->st->mu);
    owner->st->held.push_back(WsBuf{dev, *p, got, done});
  }
  GraphScratch* g = new GraphScratch{owner->st, WsBuf{dev, *p, got}};
  hipUserObject_t uo = nullptr;
  e = hipUserObjectCreate(&uo, g, graph_scratch_release, 1, hipUserObjectNoDestructorSync);
  if (e == hipSuccess) {
    {
      std::lock_guard<std::mutex> lock(owner->st->mu);
      ++owner->st->live;
    }
    e = hipGraphRetainUserObject(graph, uo, 1, hipGraphUserObjectMove);  // the graph takes our reference
    if (e != hipSuccess) (void)hipUserObjectRelease(uo, 1);                // -> destructor queues the buffer
    return e;
  }
  delete g;
  {  // back on the pending list: freed by the next uncaptured call
    std::lock_guard<std::mutex> lock(owner->st->mu);
    for (size_t i = 0; i < owner->st->held.size(); ++i)
      if (owner->st->held[i].p == *p) {
        owner->st->held.erase(owner->st->held.begin() + i);
        break;
      }
    owner->st->pending.push_back(WsBuf{dev, *p, got, done});
  }
  *p = nullptr;
  return e;
}

// the matching free: a captured solve's buffer stays with its graph, and the
// capture records its completion event after the buffer's last use (a failed
// record drops the event: that buffer is then never reused by a capture)
inline hipError_t ws_free(WsOwner* owner, void* p, hipStream_t s) {
  if (!p) return hipSuccess;
  if (owner && stream_capturing(s)) {
    std::lock_guard<std::mutex> lock(owner->st->mu);
    for (auto& b : owner->st->held)
      if (b.p == p && b.done) {
        if (hipEventRecord(b.done, s) != hipSuccess) {
          (void)hipGetLastError();
          b.reuse = false;
        }
        break;
      }
    return hipSuccess;
  }
  return hipFreeAsync(p, s);
}

// Debug knob IKG_WS_TRACE=1: every stream-ordered workspace allocation and
// free is printed (address range, whether the stream is capturing).
inline void ws_trace(const char* verb, const char* name, const void* p, size_t bytes, hipStream_t s) {
  if (!env_flag("IKG_WS_TRACE", false)) return;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &st);
  fprintf(stderr, "[ikg ws] %s %s %p +%zu -> %p%s\n", verb, name, p, bytes, (const void*)((const char*)p + bytes),
          st == hipStreamCaptureStatusActive ? " (capturing)" : "");
}

// One stream-ordered workspace: laid out by a WsLayout, allocated and traced
// once, and freed on every path out of its scope.  release() (or finish) hands
// back the free's error for the callers that report it.
// Debug knob IKG_POISON=1: the arrays are filled by their tags right after the
// allocation (adjacent arrays of one tag in one fill), so a read of memory the
// solve did not write gives a wrong answer on the first run instead of stale
// data from an earlier solve or graph replay.
class Workspace {
 public:
  Workspace(WsOwner* owner, hipStream_t s, const char* name) : owner_(owner), s_(s), name_(name) {}
  Workspace(const Workspace&) = delete;
  Workspace& operator=(const Workspace&) = delete;
  ~Workspace() { (void)release(); }

  hipError_t alloc(const WsLayout& l) {
    const hipError_t e = ws_alloc(owner_, (void**)&base_, l.total, s_);
    if (e != hipSuccess) {
      base_ = nullptr;  // (a capture that could not keep the buffer has queued it for the next drain)
      return e;
    }
    lay_ = l;
    ws_trace("alloc", name_, base_, l.total, s_);
    if (!env_flag("IKG_POISON", false)) return hipSuccess;
    for (int i = 0, j; i < l.n; i = j) {
      size_t end = l.off[i] + l.len[i];
      for (j = i + 1; j < l.n && l.fill[j] == l.fill[i] && l.off[j] == end; ++j) end += l.len[j];
      if (l.fill[i] != WsLayout::kNoFill && end > l.off[i])
        (void)hipMemsetAsync(base_ + l.off[i], l.fill[i] == WsLayout::kInt ? 0xFF : 0x7F, end - l.off[i], s_);
    }
    return hipSuccess;
  }
  explicit operator bool() const { return base_ != nullptr; }
  template <typename U>
  U* at(int i) const {
    return (U*)(base_ + lay_.off[i]);
  }
  hipError_t release() {
    if (!base_) return hipSuccess;
    ws_trace("free", name_, base_, 0, s_);
    char* p = base_;
    base_ = nullptr;
    return ws_free(owner_, p, s_);
  }
  // what a launcher returns: its launch error first, then the free's
  hipError_t finish(hipError_t e) {
    const hipError_t ef = release();
    return e != hipSuccess ? e : ef;
  }

 private:
  WsOwner* owner_;
  hipStream_t s_;
  const char* name_;
  char* base_ = nullptr;
  WsLayout lay_;
};

// Collision continuation: the buffers offered to the pair kernel, which
// records every iterate from the first passing one on (RecOut)
struct RecBufs {
  void* rec = nullptr;
  int32_t* rec_n = nullptr;
  void* ck = nullptr;         // window checkpoints (ikg_solve.hpp kWinOf), ck_per_problem per problem
  bool* rec_used = nullptr;   // set when the launch took them
  int64_t rec_slots = 0;      // records capacity: problems whose records `rec` holds (0: every problem of the launch)
};

struct BatchArgs {
  const void* targets;
  const void* q0;
  int64_t q0_stride;
  int64_t B;
  void* q_out;
  uint8_t* converged;
  int32_t* iters;
  void* err_out;
  int ppw;         // problems per 64-lane wave (1..32)
  int64_t S = 1;   // seeds per target (multi-start): problem p = (target p / S, q0 row p % S)
  int variant = 0; // ikg_variant
  // model-specialised pair kernels on this device (ikg_model_specialize), or null
  const JitKernels* jit = nullptr;
  RecBufs recs;
  // resume launch (the collision scan's windows to regenerate, ikg_collision.hip):
  // listed problems, their count (device) and windows to regenerate per problem
  const int32_t* rec_list = nullptr;
  const int32_t* rec_count = nullptr;
  const uint32_t* rec_wmask = nullptr;
  uint64_t* rec_rmask = nullptr;    // per problem and window, the iterates the resume kernel recorded
  int64_t rec_rbase = 0, rec_rcap = 0;  // list entries [rbase, rbase + rcap) this resume launch regenerates
  WsOwner* ws_owner = nullptr;  // scratch of captured solves (ws_alloc)
};

// waves of a resume launch (grid-stride over listed problems x windows)
inline unsigned resume_waves(int64_t B, int nw, int per_wave) {
  const int64_t w = (B * nw + per_wave - 1) / per_wave;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(w, 4096));
}

struct MultiArgs {
  const void* targets;
  int64_t T;
  const void* seeds;
  int64_t S;
  void* q_out;
  uint8_t* converged;
  int32_t* iters;
  void* err_out;
  int32_t* best_seed;
  int nq;
  // workspace for the S x T per-seed results (device, caller-owned)
  void* ws_q;
  uint8_t* ws_conv;
  int32_t* ws_iters;
  void* ws_err;
  // KCollision<T>* (device) when params.check_collision: the seeds' results
  // go through the collision continuation before the best-seed reduction
  const void* collision = nullptr;
  int n_geoms = 0;
  int variant = 0;  // ikg_variant of the per-seed solves
  const JitKernels* jit = nullptr;
  WsOwner* ws_owner = nullptr;
  RecBufs recs;           // for the S x T per-seed problems (BatchArgs::recs)
  int64_t rec_chunk = 0;  // targets per launch when the records of all T x S problems exceed the budget (0: all)
};

// kernel specialisation chosen at model creation (ikg_model_build.hpp)
constexpr int kSpecGeneric = 0;
constexpr int kSpecNextage = 1;
constexpr int kSpecGenericWrist = 2;  // generic tables, spherical-wrist solve

// f(DAMPED constant, Spec value) for the loop that a model's specialisation and
// the damping select; the damped solve does not use the wrist structure
template <typename F>
void by_spec(int spec, bool damped, F&& f) {
  if (spec == kSpecNextage) {
    if (damped)
      f(std::true_type{}, SpecNextage{});
    else
      f(std::false_type{}, SpecNextage{});
  } else if (damped) {
    f(std::true_type{}, SpecGeneric{});
  } else if (spec == kSpecGenericWrist) {
    f(std::false_type{}, SpecGenericWrist{});
  } else {
    f(std::false_type{}, SpecGeneric{});
  }
}

template <typename T>
hipError_t launch_pair_batch(const KModel<T>* dmodel, const KParams<T>& prm, const BatchArgs& a, int spec,
                             hipStream_t s);

// the concrete layout (IKG_VARIANT_PAIR / PACKED / QUAD) launch_pair_batch runs for B problems
template <typename T>
int resolve_variant(const KParams<T>& prm, int spec, int variant, int64_t B, bool rec);

// pair layout, Nextage specialisation, lambda = 0, built with the max-ILP
// scheduler for launches of at most one wave per SIMD (ikg_pair_ilp.hip)
hipError_t launch_pair_ilp(const KModel<float>* dmodel, const KParams<float>& prm, const BatchArgs& a, bool med,
                           size_t lds, hipStream_t s);

// packed fp32 layout, Nextage specialisation (ikg_packed.hip)
hipError_t launch_packed_batch(const KModel<float>* dmodel, const KParams<float>& prm, const BatchArgs& a,
                               hipStream_t s);

// quad layout (8 lanes per problem), Nextage specialisation (ikg_quad.hip)
template <typename T>
hipError_t launch_quad_batch(const KModel<T>* dmodel, const KParams<T>& prm, const BatchArgs& a, hipStream_t s);

template <typename T>
hipError_t launch_multistart(const KModel<T>* dmodel, const KParams<T>& prm, const MultiArgs& a, int spec,
                             hipStream_t s);

template <typename T>
hipError_t launch_fk(const KModel<T>* dmodel, const void* q, int64_t B, void* hands, hipStream_t s);

template <typename T>
hipError_t launch_log6(const void* M, int64_t B, void* out, hipStream_t s);

template <typename T>
hipError_t launch_pair_state(const KModel<T>* dm, const void* targets, const void* q0, int64_t stride, int64_t B,
                             void* out, hipStream_t s);


template <typename T>
hipError_t launch_collision(const KModel<T>* dm, const KCollision<T>* dc, const void* q, const void* targets,
                            int64_t B, uint8_t* out, hipStream_t s);

// nq / ng: model joints and scene geometries (size the per-problem LDS slices)
template <typename T>
hipError_t launch_collide_continue(const KModel<T>* dm, const KCollision<T>* dc, const KParams<T>& prm,
                                   const BatchArgs& a, int spec, int nq, int ng, hipStream_t s);

// planner queries: distance over a pair subset; target geometry
// against world-fixed geometries
template <typename T>
hipError_t launch_distance(const KModel<T>* dm, const KCollision<T>* dc, const void* q, const void* targets,
                           int64_t B, const int32_t* pair_idx, int n_idx, void* out, hipStream_t s);
template <typename T>
hipError_t launch_target_env(const KCollision<T>* dc, const void* targets, int64_t B, const int32_t* geoms,
                             int n_geoms, uint8_t* out, hipStream_t s);

// controller kinematics (ikg_control.hip): optional outputs
struct FrameKinOut {
  void* placement;  // [B,2,12]
  void* velocity;   // [B,2,6]
  void* J;          // [B,12,nq]
  void* dJ;         // [B,12,nq]
  void* dJv;        // [B,12]
  void* err;        // [B,12]
  void* derr;       // [B,12]
};
template <typename T>
hipError_t launch_frame_kin(const KModel<T>* dm, int nq, int spec, const void* q, const void* v, const void* qd,
                            const void* vd,
                            int64_t B, int rf, const FrameKinOut& o, hipStream_t s);

// controller dynamics (control.py:284-286, ikg_dynamics.hip): optional outputs
struct DynOut {
  void* M;    // [B,nq,nq]
  void* nle;  // [B,nq]
  void* g;    // [B,nq]
};
template <typename T>
hipError_t launch_dynamics(const KModel<T>* dm, const KInertia<T>* di, int nq, const void* q, const void* v,
                           int64_t B, const DynOut& o, hipStream_t s);

// controller solve (control.py:348-406, ikg_dynamics.hip): per-state inputs
// (device, fp64) and optional outputs
struct CtlIn {
  const void* M;     // [B,nq,nq]
  const void* nle;   // [B,nq]
  const void* J;     // [B,12,nq]
  const void* dJv;   // [B,12]
  const void* err;   // [B,12]
  const void* derr;  // [B,12]
};
struct CtlOut {
  void* tau;     // [B,nq]
  void* qdd;     // [B,nq]
  void* xdd;     // [B,12]
  void* Lambda;  // [B,2,36]
  void* fc;      // [B,12]
};
hipError_t launch_control_solve(const CtlIn& in, int nq, int64_t B, const KCtl<double>& prm, const CtlOut& o,
                                hipStream_t s);

// closed-loop rollout (ikg_dynamics.hip).  The two curves' control points and
// binomial factors sit in one device table: [Pq (nq_pts x nq)] [bcq (nq_pts)]
// [Pv (nv_pts x nq)] [bcv (nv_pts)].  With a curve pair per state (stride != 0)
// the table is the binomial factors alone, [bcq] [bcv], and state p's control
// points are read where the caller keeps them: pq + p stride_q, pv + p stride_v.
struct RolloutCurves {
  const double* table;
  int nq_pts, nv_pts;
  double q_tmin, q_tmax, q_mult;
  double v_tmin, v_tmax, v_mult;
  const double *pq, *pv;       // per-state control points [n, n_pts, nq], else null
  int64_t stride_q, stride_v;  // doubles between two states' curves; both 0 = one shared pair
};
IKG_HD inline size_t rollout_table_len(int nq, int nq_pts, int nv_pts, bool per_state = false) {
  return (size_t)(per_state ? 1 : nq + 1) * (nq_pts + nv_pts);
}

// Bezier trajectory fit (ikg_fit.hip): all pointers device, fp64
struct FitArgs {
  const double *q0, *q1;   // [B,dim]
  const double* y;         // packed path points [offsets[B],dim]
  const int64_t* offsets;  // [B+1]
  int dim, degree;
  double ridge, T;
  double* points;             // [B,degree+1,dim]
  double *vpoints, *apoints;  // [B,degree,dim], [B,degree-1,dim] or null
  double* cost;               // [B]
  int32_t* status;            // [B]
  double bc[21];              // bezier_coeffs(degree + 1)
};
hipError_t launch_bezier_fit(const FitArgs& args, int64_t B, hipStream_t s);

// per-tick arguments of the step kernel (device, fp64): the state rows are
// advanced in place, the desired state is rewritten for the next tick
struct StepArgs {
  void *q, *v;        // [n,nq]
  void* t;            // [n]
  void *qdes, *vdes;  // [n,nq]
  RolloutCurves cv;
  double dt_sim, dt_traj;
  void *q_hist, *v_hist, *tau_hist;  // [n,R,nq] or null
  int64_t R, slot;                   // this tick's record (slot < 0: none)
};
// dst[0..n) = host[0..n) through kernel arguments: capturable, and the host
// array is free again when the call returns
hipError_t launch_table_write(double* dst, const double* host, size_t n, hipStream_t s);
// table: [P (n_points x dim)] [bc (n_points)]; times [K] inside [t_min, t_max]
hipError_t launch_bezier_eval(const double* table, int n_points, int dim, double t_min, double t_max, double mult,
                              const double* times, int64_t K, double* out, hipStream_t s);
// nle [B,nq] from launch_dynamics; M is formed inside (about each joint's own origin)
hipError_t launch_forward_dynamics(const KModel<double>* dm, const KInertia<double>* di, int nq, const void* q,
                                   const void* nle, const void* tau, int64_t B, void* qdd, hipStream_t s);
// state <- (q0, v0, t0 or the q curve's t_min) and the desired state of tick 0
hipError_t launch_rollout_init(const void* q0, const void* v0, const void* t0, int nq, int64_t n, const StepArgs& a,
                               hipStream_t s);
hipError_t launch_control_step(const CtlIn& in, int nq, int64_t B, const KCtl<double>& prm, const StepArgs& a,
                               hipStream_t s);

}  // namespace ikg
