// Byte layouts of the stream-ordered workspaces (ikg_launch.hpp Workspace).
// Pure arithmetic, nothing from HIP: tests/ws_layout_main.cpp checks it on the CPU.
#pragma once

#include <assert.h>
#include <stddef.h>
#include <stdint.h>

namespace ikg {

// Arrays carved from one allocation in declaration order.  Each is tagged for
// IKG_POISON: integer arrays (counts, indices, flags) get 0xFF bytes (-1:
// "nothing recorded", never an index that is used); floating arrays get 0x7F
// bytes (1.4e306 / 3.4e38: finite, so no -ffinite-math-only code sees a NaN,
// but absurd as a joint angle or an error norm); kNoFill arrays are left as
// allocated.
struct WsLayout {
  enum Fill : uint8_t { kNoFill, kInt, kFloat };
  static constexpr int kMaxArrays = 8;
  size_t off[kMaxArrays] = {}, len[kMaxArrays] = {};
  Fill fill[kMaxArrays] = {};
  int n = 0;
  size_t total = 0;
  // the next array: `times` shares of `bytes`, each rounded up to a multiple of
  // `round` (256: every array starts 256-aligned); returns its index
  int add(size_t bytes, Fill f, size_t round = 256, size_t times = 1) {
    assert(n < kMaxArrays);
    off[n] = total;
    len[n] = times * ((bytes + round - 1) / round * round);
    fill[n] = f;
    total += len[n];
    return n++;
  }
  void pad(size_t bytes) { total += bytes; }  // allocated after the last array, never filled
};

// "cont", one continuation: witness / state per problem, the pre-screen's
// colliding list (or the compaction's chunk counts), the continuation's
// problems, and a 256-byte block of counts
struct ContLayout : WsLayout {
  int wit, list, clist, count;
  explicit ContLayout(size_t B)
      : wit(add(4 * B, kInt)), list(add(4 * B, kInt)), clist(add(4 * B, kInt)), count(add(256, kInt)) {}
};

// "traj", the trajectory windows: two parities of Wn records of `rec_bytes`
// each per problem, the running iterate (`q_bytes` per problem) and its
// counters (it0 and nrec per parity), the witness pair between windows
struct TrajLayout : WsLayout {
  int rec, qrun, itrun, it0, nrec, done, cst;
  TrajLayout(size_t B, size_t rec_bytes, size_t Wn, size_t q_bytes, size_t cert_bytes)
      : rec(add(2 * rec_bytes * B * Wn, kFloat)), qrun(add(q_bytes * B, kFloat)), itrun(add(4 * B, kInt)),
        it0(add(4 * B, kInt, 256, 2)), nrec(add(4 * B, kInt, 256, 2)), done(add(4 * B, kInt)),
        cst(add(cert_bytes * B, kInt)) {}
};

// "scan", the records solve's first check and scan: answered flags, the
// windows left (`mask_words` per problem), the witness pair, the recorded
// iterates per window (`windows` 64-bit masks per problem) and the split
// scan's best / arrive, which are allocated always and filled only when the
// split scan is on (the first check sets them for every problem it may list)
struct ScanLayout : WsLayout {
  int done, wmask, cst, rmask, best, arrive;
  ScanLayout(size_t B, size_t mask_words, size_t cert_bytes, size_t windows, bool split)
      : done(add(4 * B, kInt)), wmask(add(4 * mask_words * B, kInt)), cst(add(cert_bytes * B, kInt)),
        rmask(add(8 * windows * B, kInt)), best(add(4 * B, split ? kInt : kNoFill)),
        arrive(add(4 * B, split ? kInt : kNoFill)) {}
};

// "rec", the batch kernel's records: regenerated records for `slots` problems,
// checkpoints and record counts for all n (the counts filled to their exact
// length, the rounding after them left alone)
struct RecLayout : WsLayout {
  int rec, ck, rec_n;
  RecLayout(size_t n, size_t slots, size_t records_bytes, size_t ck_bytes)
      : rec(add(records_bytes * slots, kFloat)), ck(add(ck_bytes * n, kFloat)), rec_n(add(4 * n, kInt, 1)) {
    pad((256 - 4 * n % 256) % 256);
  }
};

// "multistart", the per-seed results of n = targets x seeds problems, packed
// (`elem` bytes per value), with 64 spare bytes
struct MultiLayout : WsLayout {
  int q, err, iters, conv;
  MultiLayout(size_t n, size_t elem, size_t nq)
      : q(add(elem * nq * n, kFloat, 1)), err(add(elem * 2 * n, kFloat, 1)), iters(add(4 * n, kInt, 1)),
        conv(add(n, kInt, 1)) {
    pad(64);
  }
};

}  // namespace ikg
