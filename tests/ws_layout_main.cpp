// Stand-alone check of csrc/ikg_ws_layout.hpp (tests/test_ws_layout.py builds it
// with -fsanitize=address,undefined and runs it): the six workspaces' arrays
// ascend without overlap, start 256-aligned where the workspace is aligned, and
// each total equals a literal worked out by hand from the formulas the
// launchers used before the layouts were shared.
//
// Sizes: nq = 15, max_iters = 1,000, elem = 8 (fp64) or 4 (fp32), and from the
// kernel headers
//   rec_len     = 16 + ((nq - 13 + 3) & ~3)   = 20 values per record
//   rec_windows = 1000 / 32 + 1               = 32 windows (fp64 and fp32)
//   mask_words  = (32 + 31) / 32              = 1
//   ck          = (32 + 2) * 64               = 2,176 values per problem
//   sizeof(TrajCert) = 4 bytes
// al(x) rounds x up to a multiple of 256; al(4 B) = 256, 256, 16,384 for
// B = 1, 63, 4,096.
#include <stdio.h>
#include <stdlib.h>

#include "ikg_ws_layout.hpp"

using namespace ikg;

static int g_bad = 0;

static void check(const char* name, size_t B, int elem, const WsLayout& l, size_t want_total, bool aligned) {
  bool ok = l.total == want_total && l.n > 0 && l.off[0] == 0;
  for (int i = 0; i < l.n; ++i) {
    const size_t end = l.off[i] + l.len[i];
    if (aligned && l.off[i] % 256) ok = false;
    if (end > (i + 1 < l.n ? l.off[i + 1] : l.total)) ok = false;  // overlap, or past the allocation
    if (i + 1 < l.n && l.off[i + 1] < l.off[i]) ok = false;
  }
  if (!ok) {
    ++g_bad;
    fprintf(stderr, "%s B=%zu elem=%d: total %zu (want %zu);", name, B, elem, l.total, want_total);
    for (int i = 0; i < l.n; ++i) fprintf(stderr, " [%zu +%zu]", l.off[i], l.len[i]);
    fprintf(stderr, "\n");
  }
}

static void expect(bool ok, const char* what) {
  if (ok) return;
  ++g_bad;
  fprintf(stderr, "%s\n", what);
}

int main() {
  const size_t Bs[3] = {1, 63, 4096};
  const int elems[2] = {8, 4};
  const size_t RL = 20, WINDOWS = 32, MASK_WORDS = 1, CK = 2176, CERT = 4, NQ = 15, FULL = 1001;

  // cont: 3 al(4 B) + 256  (wit, list, clist; count), the same in fp64 and fp32
  //   B = 1: 768 + 256; B = 63: 768 + 256; B = 4,096: 49,152 + 256
  const size_t cont[3] = {1024, 1024, 49408};
  // scan: 5 al(4 B) + al(8 * 32 * B)  (done, wmask, cst, best, arrive; rmask), the same in fp64 and fp32
  //   B = 1: 1,280 + 256; B = 63: 1,280 + 16,128; B = 4,096: 81,920 + 1,048,576
  const size_t scan[3] = {1536, 17408, 1130496};
  // traj: al(2 * 20 * elem * B * 128) + al(elem * 15 * B) + 7 al(4 B); the window is 128 iterates at these sizes
  // (4 GiB / (2 * 20 * 8 * 4,096) = 3,276 > 128)
  //   B = 1:     40,960 + 256 + 1,792 = 43,008            | 20,480 + 256 + 1,792 = 22,528
  //   B = 63:    2,580,480 + al(7,560) = 7,680 + 1,792 = 2,589,952 | 1,290,240 + al(3,780) = 3,840 + 1,792 = 1,295,872
  //   B = 4,096: 167,772,160 + 491,520 + 114,688 = 168,378,368 | 83,886,080 + 245,760 + 114,688 = 84,246,528
  const size_t traj[3][2] = {{43008, 22528}, {2589952, 1295872}, {168378368, 84246528}};
  // rec, every problem's records held (1 GiB / 160,160 = 6,704 >= 4,096 slots):
  // al(elem * 20 * 1,001 * n) + al(elem * 2,176 * n) + al(4 n); a problem's records take 160,160 | 80,080 bytes,
  // its checkpoints 17,408 | 8,704
  //   n = 1:     160,256 + 17,408 + 256 = 177,920        | 80,128 + 8,704 + 256 = 89,088
  //   n = 63:    al(10,090,080) = 10,090,240 + 1,096,704 + 256 = 11,187,200 | al(5,045,040) = 5,045,248 + 548,352 + 256 = 5,593,856
  //   n = 4,096: 656,015,360 + 71,303,168 + 16,384 = 727,334,912 | 328,007,680 + 35,651,584 + 16,384 = 363,675,648
  const size_t rec[3][2] = {{177920, 89088}, {11187200, 5593856}, {727334912, 363675648}};
  // rec with a 4 MiB records budget, n = 4,096: slots = 4,194,304 / 160,160 = 26 | / 80,080 = 52, both
  // 4,164,160 bytes of records -> al = 4,164,352; + 71,303,168 | 35,651,584 + 16,384
  const size_t rec_small[2] = {75483904, 39832320};
  // multistart, n problems: n * (15 elem + 2 elem + 4 + 1) + 64 = 141 n + 64 | 73 n + 64
  const size_t multi[3][2] = {{205, 137}, {8947, 4663}, {577600, 299072}};

  for (int b = 0; b < 3; ++b)
    for (int e = 0; e < 2; ++e) {
      const size_t B = Bs[b], el = (size_t)elems[e], ib = (4 * B + 255) / 256 * 256;
      const ContLayout c(B);
      check("cont", B, elems[e], c, cont[b], true);
      expect(c.n == 4 && c.off[c.wit] == 0 && c.off[c.list] == ib && c.off[c.clist] == 2 * ib &&
                 c.off[c.count] == 3 * ib && c.len[c.count] == 256,
             "cont: array order");
      for (int split = 0; split < 2; ++split) {
        const ScanLayout s(B, MASK_WORDS, CERT, WINDOWS, split != 0);
        check("scan", B, elems[e], s, scan[b], true);
        expect(s.fill[s.best] == (split ? WsLayout::kInt : WsLayout::kNoFill) && s.fill[s.arrive] == s.fill[s.best] &&
                   s.fill[s.done] == WsLayout::kInt && s.off[s.arrive] == s.off[s.best] + ib,
               "scan: best / arrive are filled only with the split scan");
      }
      const TrajLayout t(B, RL * el, 128, el * NQ, CERT);
      check("traj", B, elems[e], t, traj[b][e], true);
      expect(t.off[t.nrec] - t.off[t.it0] == 2 * ib && t.off[t.done] - t.off[t.nrec] == 2 * ib &&
                 t.fill[t.qrun] == WsLayout::kFloat && t.fill[t.itrun] == WsLayout::kInt,
             "traj: it0 and nrec hold two parities");
      const RecLayout r(B, B, el * RL * FULL, el * CK);
      check("rec", B, elems[e], r, rec[b][e], true);
      expect(r.len[r.rec_n] == 4 * B, "rec: the counts are filled to their exact length");
      const MultiLayout m(B, el, NQ);
      check("multistart", B, elems[e], m, multi[b][e], false);
      expect(m.off[m.err] == el * NQ * B && m.off[m.conv] + B + 64 == m.total, "multistart: packed, 64 spare bytes");
    }
  for (int e = 0; e < 2; ++e) {
    const size_t el = (size_t)elems[e], per = el * RL * FULL, slots = ((size_t)4 << 20) / per;
    expect(slots == (e == 0 ? 26u : 52u) && slots < 4096, "rec: slots under a 4 MiB budget");
    check("rec (4 MiB records budget)", 4096, elems[e], RecLayout(4096, slots, per, el * CK), rec_small[e], true);
  }
  // the controller's scratch: one packed fp64 array, 15 * 15 + 12 * 15 + 15 + 36 = 456 values per state
  for (int b = 0; b < 3; ++b) {
    WsLayout l;
    l.add(8 * 456 * Bs[b], WsLayout::kFloat, 1);
    const size_t want[3] = {3648, 229824, 14942208};
    check("controller", Bs[b], 8, l, want[b], false);
  }
  if (g_bad) return 1;
  printf("ws layout ok\n");
  return 0;
}
