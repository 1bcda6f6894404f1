// Host check of etcd_amd/csrc/lead_prop_step.h, the decisions the kernels of
// elead_local_batch_device share with this program:
//   1. random runs from a fixed seed: the closed form of every record of a
//      closed() run against the serial step, record for record (result,
//      entry, messages) and the run's final state;
//   2. the case files given as arguments (written by the pytest from the
//      Python checker): the serial step against the checker's outcome.
// Prints the records per outcome class, then "ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lead_prop_step.h"

namespace lp = lead_prop;

struct Rng {   // splitmix64
  uint64_t x;
  uint64_t next() {
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
  bool chance(uint32_t pct) { return below(100) < pct; }
};

struct Emitted {
  uint64_t w[8];   // kind (0 entry, 1 message), then the fields
  bool operator==(const Emitted &o) const { return memcmp(w, o.w, sizeof w) == 0; }
};

struct Sink {
  std::vector<Emitted> out;
  void entry(uint64_t pos, uint64_t term, uint64_t index) { out.push_back(Emitted{{0, pos, term, index, 0, 0, 0, 0}}); }
  void msg(uint64_t j, const lp::State &s, const lp::Msg &m) {
    // from / term ride on the state; fold them into the comparison through `to`'s neighbours
    out.push_back(Emitted{{1 + j, m.type, m.to, m.index, m.log_term, m.commit ^ (s.id << 1) ^ (s.term << 33), m.efirst, m.nents}});
  }
};

struct TermAt {
  const std::vector<uint64_t> *terms;
  uint64_t operator()(uint64_t pos) const {
    if (pos >= terms->size()) {
      fprintf(stderr, "term_at(%" PRIu64 ") past the %zu old entries\n", pos, terms->size());
      exit(1);
    }
    return (*terms)[pos];
  }
};

static bool same_out(const lp::Out &a, const lp::Out &b) {
  return a.status == b.status && a.action == b.action && a.n_msgs == b.n_msgs && a.index == b.index && a.pos == b.pos &&
         a.committed == b.committed;
}

static bool same_state(const lp::State &a, const lp::State &b) {
  bool ok = a.committed == b.committed && a.nlog == b.nlog && a.unstable == b.unstable && a.pending == b.pending;
  for (uint32_t k = 0; k < lp::PEERS; ++k) ok = ok && a.match[k] == b.match[k] && a.next[k] == b.next[k];
  return ok;
}

static uint64_t classes[5];

struct Rec {
  uint64_t kind;
  int32_t etype;
};

// the serial replay of one run, as the kernels' head lane does it
static void serial_run(lp::State &s, const std::vector<uint64_t> &terms, const std::vector<Rec> &recs,
                       std::vector<lp::Out> &outs, std::vector<std::vector<Emitted>> &emits) {
  const TermAt term_at{&terms};
  bool stopped = false;
  const bool unsupported = s.np > lp::PEERS;
  for (const Rec &r : recs) {
    lp::Out o;
    Sink sink;
    if (stopped || unsupported) {
      o.status = stopped ? lp::ST_OK : lp::ST_UNSUPPORTED;
      o.action = stopped ? lp::NOT_STEPPED : lp::PANICKED;
      o.n_msgs = o.index = o.pos = 0;
      o.committed = s.committed;
      stopped = true;
    } else {
      o = lp::step<true>(s, r.kind, r.etype, term_at, sink);
    }
    stopped = stopped || o.status != lp::ST_OK;
    outs.push_back(o);
    emits.push_back(sink.out);
  }
}

static int random_runs(uint64_t runs) {
  Rng g{20260704};
  uint64_t closed_runs = 0;
  for (uint64_t it = 0; it < runs; ++it) {
    lp::State s;
    memset(&s, 0, sizeof s);
    const uint64_t np = g.chance(3) ? 0 : g.chance(3) ? 8 : 1 + g.below(7);
    static const uint64_t offs[] = {0, 0, 5, 100, 0xFFFFFFFFFFFFFFF0ull, (1ull << 62) + 77};
    s.off = offs[g.below(g.chance(4) ? 6 : 4)];
    s.nlog = g.chance(3) ? 0 : 1 + g.below(12);
    s.np = np;
    s.term = g.chance(2) ? 0 : 1 + g.below(3);
    std::vector<uint64_t> terms(s.nlog);
    uint64_t t = g.below(2);
    for (auto &x : terms) {
      if (g.chance(30) && t < s.term) ++t;
      x = t;
    }
    const uint64_t last = s.nlog - 1 + s.off;
    const uint64_t slots = np < lp::PEERS ? np : lp::PEERS;
    for (uint64_t k = 0; k < slots; ++k) {
      s.pid[k] = 10 + k;
      // matches and nexts on both sides of the log's ends
      s.match[k] = g.chance(40) ? 0 : s.off + g.below(s.nlog + 3) - (g.chance(10) ? 2 : 0);
      const uint32_t how = (uint32_t)g.below(20);
      s.next[k] = how == 0 ? s.off : how == 1 ? s.off - 1 : how == 2 ? last + 2 + g.below(3) : how == 3 ? 0
                  : s.off + 1 + g.below(s.nlog + 1);
    }
    s.id = (slots && !g.chance(4)) ? s.pid[g.below(slots)] : 999;
    s.committed = s.off + g.below(s.nlog + 1);
    s.unstable = g.chance(50) ? last + 1 - g.below(3) : last + 1 + g.below(5);
    s.pending = g.below(2);
    s.fresh = s.nlog;
    s.snap_ok = g.chance(80);
    s.efirst = 0;
    std::vector<Rec> recs(1 + g.below(g.chance(10) ? 40 : 6));
    for (Rec &r : recs) {
      r.kind = g.chance(25) ? lp::KIND_BEAT : lp::KIND_PROP;
      r.etype = g.chance(35) ? 1 : 0;
    }
    const lp::State s0 = s;
    const lp::Run run = lp::prepare(s0);
    std::vector<lp::Out> outs;
    std::vector<std::vector<Emitted>> emits;
    serial_run(s, terms, recs, outs, emits);
    for (const lp::Out &o : outs) ++classes[o.action];
    if (!run.closed) continue;
    ++closed_runs;
    const TermAt term_at{&terms};
    uint64_t nprops = 0, ncc = 0;
    for (size_t j = 0; j < recs.size(); ++j) {
      nprops += recs[j].kind == lp::KIND_PROP;
      ncc += recs[j].kind == lp::KIND_PROP && recs[j].etype == 1;
      Sink sink;
      const lp::Out o = lp::closed_record<true>(s0, run, recs[j].kind, recs[j].etype, nprops, ncc, term_at, sink);
      Sink none;
      const lp::Out o2 = lp::closed_record<false>(s0, run, recs[j].kind, recs[j].etype, nprops, ncc, term_at, none);
      if (!same_out(o, outs[j]) || !same_out(o2, outs[j]) || !(sink.out == emits[j]) || !none.out.empty()) {
        fprintf(stderr, "run %" PRIu64 " record %zu: the closed form differs (action %d / %d, committed %" PRIu64
                        " / %" PRIu64 ", index %" PRIu64 " / %" PRIu64 ")\n",
                it, j, o.action, outs[j].action, o.committed, outs[j].committed, o.index, outs[j].index);
        return 1;
      }
    }
    const lp::State e = lp::closed_state(s0, run, lp::accepted_upto(s0, nprops, ncc), ncc > 0, term_at);
    if (!same_state(e, s)) {
      fprintf(stderr, "run %" PRIu64 ": the closed form's final state differs\n", it);
      return 1;
    }
  }
  printf("runs %" PRIu64 " closed %" PRIu64 "\n", runs, closed_runs);
  return closed_runs * 3 < runs ? 1 : 0;   // the generator must keep most runs in the closed form's domain
}

// A case file: whitespace-separated unsigned integers.
//   n_cases, then per case:
//     id term committed off nlog np  pid[7] match[7] next[7]  unstable pending snap_ok
//     terms[nlog]
//     n_records, per record: kind etype | status action n_msgs index pos committed
//                            n_emitted, per emitted: 0 pos term index | 1 type to index log_term commit efirst nents
//     the final state: committed nlog unstable pending match[7] next[7]
static int case_file(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) {
    perror(path);
    return 1;
  }
  auto rd = [&]() -> uint64_t {
    uint64_t v = 0;
    if (fscanf(f, "%" SCNu64, &v) != 1) {
      fprintf(stderr, "%s: short file\n", path);
      exit(1);
    }
    return v;
  };
  const uint64_t n_cases = rd();
  for (uint64_t c = 0; c < n_cases; ++c) {
    lp::State s;
    memset(&s, 0, sizeof s);
    s.id = rd(), s.term = rd(), s.committed = rd(), s.off = rd(), s.nlog = rd(), s.np = rd();
    for (auto &x : s.pid) x = rd();
    for (auto &x : s.match) x = rd();
    for (auto &x : s.next) x = rd();
    s.unstable = rd(), s.pending = rd(), s.snap_ok = rd() != 0;
    s.fresh = s.nlog;
    std::vector<uint64_t> terms(s.nlog);
    for (auto &x : terms) x = rd();
    const uint64_t n_recs = rd();
    std::vector<Rec> recs(n_recs);
    std::vector<lp::Out> want(n_recs);
    std::vector<std::vector<Emitted>> want_emits(n_recs);
    for (uint64_t j = 0; j < n_recs; ++j) {
      recs[j].kind = rd(), recs[j].etype = (int32_t)rd();
      lp::Out &o = want[j];
      o.status = (int32_t)rd(), o.action = (int32_t)rd(), o.n_msgs = rd(), o.index = rd(), o.pos = rd(), o.committed = rd();
      const uint64_t n_em = rd();
      uint64_t j_msg = 0;
      for (uint64_t k = 0; k < n_em; ++k) {
        Emitted e{{0, 0, 0, 0, 0, 0, 0, 0}};
        if (rd() == 0) {
          e.w[1] = rd(), e.w[2] = rd(), e.w[3] = rd();
        } else {
          e.w[0] = 1 + j_msg++;
          for (int x = 1; x < 8; ++x) e.w[x] = rd();
          e.w[5] ^= (s.id << 1) ^ (s.term << 33);
        }
        want_emits[j].push_back(e);
      }
    }
    std::vector<lp::Out> outs;
    std::vector<std::vector<Emitted>> emits;
    serial_run(s, terms, recs, outs, emits);
    for (uint64_t j = 0; j < n_recs; ++j)
      if (!same_out(outs[j], want[j]) || !(emits[j] == want_emits[j])) {
        fprintf(stderr, "%s case %" PRIu64 " record %" PRIu64 ": status %d / %d action %d / %d n_msgs %" PRIu64
                        " / %" PRIu64 " index %" PRIu64 " / %" PRIu64 " pos %" PRIu64 " / %" PRIu64
                        " committed %" PRIu64 " / %" PRIu64 " emitted %zu / %zu\n",
                path, c, j, outs[j].status, want[j].status, outs[j].action, want[j].action, outs[j].n_msgs,
                want[j].n_msgs, outs[j].index, want[j].index, outs[j].pos, want[j].pos, outs[j].committed,
                want[j].committed, emits[j].size(), want_emits[j].size());
        return 1;
      }
    lp::State e = s;
    e.committed = rd(), e.nlog = rd(), e.unstable = rd(), e.pending = rd();
    for (auto &x : e.match) x = rd();
    for (auto &x : e.next) x = rd();
    if (!same_state(e, s)) {
      fprintf(stderr, "%s case %" PRIu64 ": the final state differs\n", path, c);
      return 1;
    }
  }
  fclose(f);
  printf("%s: %" PRIu64 " cases\n", path, n_cases);
  return 0;
}

int main(int argc, char **argv) {
  if (random_runs(120000)) return 1;
  for (int k = 1; k < argc; ++k)
    if (case_file(argv[k])) return 1;
  printf("classes not_stepped=%" PRIu64 " beat=%" PRIu64 " appended=%" PRIu64 " dropped=%" PRIu64 " panicked=%" PRIu64
         "\n",
         classes[0], classes[1], classes[2], classes[3], classes[4]);
  printf("ok\n");
  return 0;
}
