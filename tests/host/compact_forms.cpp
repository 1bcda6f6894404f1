// compact_forms.cpp -- the host check of etcd_amd/csrc/compact_step.h: the
// decision the kernels of compact_step.hip run, compiled for the host, over
// random requests drawn by the generator tests/compact_cases.py restates draw
// for draw (draw).  The requests are taken a batch of 256 at a time, as a
// workgroup of the counting pass takes them: every request is decided on the
// log as the batch found it, its move descriptor and the two classes' exclusive
// scans are built, and then the entries travel as the move pass moves them --
// one "lane" per moved entry that finds its descriptor by a search in the
// scanned offsets; the disjoint class in place, the overlapping class through
// a staging array, every read before the first write; the lanes run in
// descending order, so nothing here leans on an order among them.  The digest
// of every outcome, final record, snapshot and whole window is printed for the
// Python restatement (which keeps a real list of entries and reslices it) to
// reproduce.
//
//   compact_forms <seed> <runs>
//   -> "runs N", "classes not_stepped=.. not_due=.. compacted=.. panicked=..", "statuses ok=.. ...",
//      "moves none=.. disjoint=.. overlap=..", "digest H", "ok"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "compact_step.h"

namespace cs = compact_step;
namespace lp = lead_prop;

struct SplitMix {
  uint64_t x;
  SplitMix(uint64_t seed, uint64_t run) : x(seed * 0x9E3779B97F4A7C15ull + run) {}
  uint64_t next() {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t rnd(uint64_t n) { return next() % n; }
};

static const uint64_t OFF_TABLE[6] = {0, 0, 5, 1000, ~0ull - 7, 0};
static const uint64_t NLOG_TABLE[8] = {0, 1, 2, 3, 6, 9, 20, 70};
static const uint64_t ROOM = 4, CANARY = 0xC0FFEE00DEADBEEFull, THRESHOLD = 10000;

struct Case {
  lp::State s;
  uint64_t applied;
  cs::Req q;
  uint64_t snap[6];                // data_off, data_len, nodes_off, n_nodes, removed_off, n_removed
  std::vector<uint64_t> terms;
};

static Case draw(uint64_t seed, uint64_t run) {
  SplitMix r(seed, run);
  Case c;
  lp::State &s = c.s;
  s = lp::State{};
  s.off = OFF_TABLE[r.rnd(6)];
  s.nlog = NLOG_TABLE[r.rnd(8)];
  uint64_t t = 1 + r.rnd(3);
  for (uint64_t k = 0; k < s.nlog; ++k) {
    t += r.rnd(3) == 0 ? 1 : 0;
    c.terms.push_back(t);
  }
  const uint64_t last = s.off + s.nlog - 1;
  const uint64_t amode = r.rnd(8);
  if (amode == 0)
    c.applied = s.off - 1 - r.rnd(2);
  else if (amode == 1)
    c.applied = last + 1 + r.rnd(3);
  else
    c.applied = s.off + r.rnd(s.nlog + 1);
  s.unstable = s.off + r.rnd(s.nlog + 3);
  s.id = 1;
  s.term = t;
  s.committed = c.applied;
  s.np = 1;
  s.pid[0] = 1;
  s.next[0] = 1;
  s.fresh = s.nlog;
  const bool at = r.rnd(3) == 0;
  c.q = cs::Req{at ? cs::AT_APPLIED : 0, 0, 0};
  if (at) {
    const uint64_t tmode = r.rnd(4);
    c.q.threshold = tmode == 0 ? 0 : tmode == 1 ? c.applied - s.off : tmode == 2 ? c.applied - s.off - 1 : THRESHOLD;
  } else {
    const uint64_t imode = r.rnd(8);
    c.q.index = imode == 0   ? c.applied + 1
                : imode == 1 ? s.off - 1
                : imode == 2 ? s.off
                : imode == 3 ? c.applied
                             : s.off + r.rnd(s.nlog + 1);
  }
  for (int k = 0; k < 6; ++k) {
    static const uint64_t mod[6] = {100, 50, 8, 4, 8, 3};
    c.snap[k] = r.rnd(mod[k]);
  }
  return c;
}

static uint64_t g_hash = 0xCBF29CE484222325ull;
static void fold(uint64_t v) { g_hash = (g_hash ^ v) * 0x100000001B3ull; }

struct Move {
  uint64_t cnt, cls, src, dst, loc_d, loc_o;
};

[[noreturn]] static void fail(const char *what, uint64_t run) {
  std::printf("FAIL: run %llu: %s\n", (unsigned long long)run, what);
  std::exit(1);
}

// the last k with loc(k) <= x, as the move pass searches
template <class Loc>
static size_t last_le(size_t m, uint64_t x, const Loc &loc) {
  size_t lo = 0, hi = m;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (loc(mid) <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("usage: compact_forms <seed> <runs>\n");
    return 2;
  }
  const uint64_t seed = std::strtoull(argv[1], nullptr, 10), runs = std::strtoull(argv[2], nullptr, 10);
  uint64_t classes[4] = {0}, statuses[5] = {0}, moves[3] = {0};
  for (uint64_t j0 = 0; j0 < runs; j0 += 256) {
    const uint64_t nb = std::min<uint64_t>(256, runs - j0);
    std::vector<Case> cases;
    std::vector<uint64_t> ents, cap;
    for (uint64_t k = 0; k < nb; ++k) {
      Case c = draw(seed, j0 + k);
      c.s.efirst = ents.size();
      ents.insert(ents.end(), c.terms.begin(), c.terms.end());
      ents.insert(ents.end(), ROOM, CANARY);
      cap.push_back(c.s.nlog + ROOM);
      cases.push_back(c);
    }
    // the counting pass: decisions and descriptors on the log as the batch found it
    std::vector<cs::Out> outs;
    std::vector<Move> mv;
    uint64_t nd = 0, no = 0;
    for (uint64_t k = 0; k < nb; ++k) {
      const Case &c = cases[k];
      const cs::Out o = cs::decide(c.s, c.applied, c.q, [&](uint64_t pos) { return ents.at(c.s.efirst + pos); });
      Move m{0, cs::MOVE_NONE, 0, 0, nd, no};
      if (o.action == cs::COMPACTED) {
        if (o.n_left > c.s.nlog || o.shift != c.s.nlog - o.n_left) fail("the survivors are not the log's tail", j0 + k);
        m.cls = cs::move_class(o.n_left, o.shift);
        m.cnt = m.cls == cs::MOVE_NONE ? 0 : o.n_left;
        m.src = c.s.efirst + o.shift;
        m.dst = c.s.efirst;
      } else if (o.index | o.term | o.n_left | o.shift | o.unstable) {
        fail("a request that did not compact reports something", j0 + k);
      }
      nd += m.cls == cs::MOVE_DISJOINT ? m.cnt : 0;
      no += m.cls == cs::MOVE_OVERLAP ? m.cnt : 0;
      outs.push_back(o);
      mv.push_back(m);
    }
    // the move pass, one lane per moved entry, the lanes in descending order
    const auto lane = [&](uint64_t r, bool ov, uint64_t *pos) {
      const size_t idx = last_le(mv.size(), r, [&](size_t k) { return ov ? mv[k].loc_o : mv[k].loc_d; });
      const Move &m = mv[idx];
      const uint64_t k = r - (ov ? m.loc_o : m.loc_d);
      if (k >= m.cnt || m.cls != (ov ? cs::MOVE_OVERLAP : cs::MOVE_DISJOINT)) fail("the search found no descriptor", j0);
      pos[0] = m.src + k;
      pos[1] = m.dst + k;
    };
    uint64_t pos[2];
    for (uint64_t r = nd; r-- > 0;) {
      lane(r, false, pos);
      ents.at(pos[1]) = ents.at(pos[0]);
    }
    std::vector<uint64_t> stage(no);
    for (uint64_t r = no; r-- > 0;) {
      lane(r, true, pos);
      stage.at(r) = ents.at(pos[0]);
    }
    for (uint64_t r = no; r-- > 0;) {
      lane(r, true, pos);
      ents.at(pos[1]) = stage.at(r);
    }
    // the applying pass's words and the digest, in run order
    for (uint64_t k = 0; k < nb; ++k) {
      const Case &c = cases[k];
      const cs::Out &o = outs[k];
      const bool done = o.action == cs::COMPACTED;
      classes[o.action]++;
      statuses[o.status == 0 ? 0 : o.status == 33 ? 1 : o.status == 45 ? 2 : o.status == 46 ? 3 : 4]++;
      if (done) moves[mv[k].cls]++;
      fold((uint64_t)(int64_t)o.status), fold((uint64_t)o.action), fold(o.index), fold(o.term), fold(o.n_left);
      fold(o.shift), fold(o.unstable), fold(mv[k].cls);
      fold(done ? o.index : c.s.off), fold(done ? o.n_left : c.s.nlog), fold(done ? o.unstable : c.s.unstable);
      fold(done ? o.index : 0), fold(done ? o.term : 0);
      for (int w = 0; w < 6; ++w) fold(done ? c.snap[w] : 0);
      for (uint64_t w = 0; w < cap[k]; ++w) fold(ents.at(c.s.efirst + w));
    }
  }
  static const char *names[4] = {"not_stepped", "not_due", "compacted", "panicked"};
  static const char *snames[5] = {"ok", "bounds", "compact_applied", "compact_bounds", "unsupported"};
  static const char *mnames[3] = {"none", "disjoint", "overlap"};
  std::printf("runs %llu\nclasses", (unsigned long long)runs);
  for (int k = 0; k < 4; ++k) std::printf(" %s=%llu", names[k], (unsigned long long)classes[k]);
  std::printf("\nstatuses");
  for (int k = 0; k < 5; ++k) std::printf(" %s=%llu", snames[k], (unsigned long long)statuses[k]);
  std::printf("\nmoves");
  for (int k = 0; k < 3; ++k) std::printf(" %s=%llu", mnames[k], (unsigned long long)moves[k]);
  std::printf("\ndigest %llu\nok\n", (unsigned long long)g_hash);
  return 0;
}
