// vote_step_forms.cpp -- the host check of etcd_amd/csrc/vote_step.h: the
// serial election step the kernels of vote_step.hip run, compiled for the
// host, over random runs drawn by the generator tests/vote_step_cases.py
// restates draw for draw (random_run).  Every run is replayed twice, as the
// kernels do -- counting (EMIT false), then applying (EMIT true) -- with the
// run's own entries kept aside as vote_step.hip keeps them; the two replays
// must agree, and the digest of every outcome, message, entry and final record
// is printed for the Python restatement to reproduce.
//
//   vote_step_forms <seed> <runs>
//   -> "runs N records M", "classes not_stepped=.. ... panicked=..", "digest H", "ok"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vote_step.h"

namespace vs = vote_step;
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

static const uint64_t NP_TABLE[16] = {1, 2, 2, 3, 3, 3, 3, 4, 5, 5, 5, 7, 3, 2, 0, 8};
static const uint64_t OFF_TABLE[6] = {0, 0, 5, 1000, ~0ull - 1, ~0ull - 1};
static const uint64_t STATE_TABLE[6] = {0, 0, 1, 1, 1, 2};
static const uint64_t KIND_TABLE[6] = {0, 5, 5, 6, 6, 6};

struct Case {
  lp::State s;
  vs::Vote v;
  std::vector<uint64_t> terms;
  std::vector<int32_t> types;
  std::vector<vs::Rec> recs;
};

static Case draw(uint64_t seed, uint64_t run) {
  SplitMix r(seed, run);
  Case c;
  lp::State &s = c.s;
  s = lp::State{};
  s.np = NP_TABLE[r.rnd(16)];
  const uint64_t slots = s.np < 7 ? s.np : 7;
  s.off = OFF_TABLE[r.rnd(6)];
  s.nlog = r.rnd(8);
  uint64_t t = 1 + r.rnd(3);
  for (uint64_t k = 0; k < s.nlog; ++k) {
    t += r.rnd(3) == 0 ? 1 : 0;
    c.terms.push_back(t);
    c.types.push_back(r.rnd(3) == 0 ? 1 : 0);
  }
  s.term = t + r.rnd(2);
  s.committed = s.off + (r.rnd(2) ? r.rnd(s.nlog + 1) : 0);
  if (r.rnd(8) == 0) s.committed = s.off - 1;
  for (uint64_t k = 0; k < slots; ++k) s.pid[k] = 10 + 3 * k + r.rnd(3);
  const uint64_t me = slots ? r.rnd(slots) : 0;
  s.id = slots ? s.pid[me] : 10;
  if (r.rnd(5) == 0) s.id = 999;
  for (uint64_t k = 0; k < slots; ++k) {
    const uint64_t match = s.off + r.rnd(s.nlog + 1), roll = r.rnd(10);
    s.match[k] = match;
    s.next[k] = roll == 0 ? s.off : roll == 1 ? s.off - 1 : match + 1;
  }
  c.v.state = STATE_TABLE[r.rnd(6)];
  const uint64_t vote_of[3] = {0, slots ? s.pid[r.rnd(slots)] : 0, 77};
  c.v.vote = vote_of[r.rnd(3)];
  c.v.lead = r.rnd(2) * s.id;
  c.v.elapsed = r.rnd(10);
  c.v.voted = c.v.granted = 0;
  if (c.v.state == vs::CANDIDATE) {
    c.v.voted = r.next() & ((1ull << slots) - 1);
    c.v.granted = c.v.voted & r.next();
  }
  s.unstable = s.off + r.rnd(s.nlog + 3);
  s.pending = r.rnd(2);
  s.snap_ok = r.rnd(2) != 0;
  s.efirst = 0;
  s.fresh = s.nlog;
  uint64_t cur = s.term;
  const uint64_t nrec = 1 + r.rnd(6);
  for (uint64_t j = 0; j < nrec; ++j) {
    vs::Rec m;
    m.kind = KIND_TABLE[r.rnd(6)];
    m.from = 55;
    if (slots) {                                     // Python: ids[r.rnd(slots)] if slots and r.rnd(8) else 55
      if (r.rnd(8)) m.from = s.pid[r.rnd(slots)];
    }
    const uint64_t rel = r.rnd(8);
    m.term = rel == 0 ? 0 : rel == 1 ? cur - 1 : rel == 7 ? cur + 2 : cur + (r.rnd(4) == 0 ? 1 : 0);
    cur = m.kind == vs::KIND_HUP ? cur + 1 : (m.term > cur ? m.term : cur);
    m.index = s.off + r.rnd(s.nlog + 2);
    m.log_term = r.rnd(t + 2);
    m.reject = r.rnd(4) == 0;
    c.recs.push_back(m);
  }
  return c;
}

struct TermAt {
  const std::vector<uint64_t> *old, *own;
  uint64_t first;
  uint64_t operator()(uint64_t pos) const { return pos >= first ? (*own)[pos - first] : (*old)[pos]; }
};
struct TypeAt {
  const std::vector<int32_t> *old;
  uint64_t first;
  int32_t operator()(uint64_t pos) const { return pos >= first ? 0 : (*old)[pos]; }
};

struct Emitted {
  uint64_t w[8];
};
struct Sink {
  std::vector<Emitted> msgs;
  uint64_t ent[3] = {~0ull, ~0ull, ~0ull};
  void put(uint64_t j, const Emitted &e) {
    if (msgs.size() <= j) msgs.resize(j + 1);
    msgs[j] = e;
  }
  void entry(uint64_t pos, uint64_t term, uint64_t index) { ent[0] = pos, ent[1] = term, ent[2] = index; }
  void msg(uint64_t j, const lp::State &, const lp::Msg &m) {
    put(j, Emitted{{m.type, m.to, m.index, m.log_term, m.commit, m.nents ? m.efirst : 0, m.nents, 0}});
  }
  void vote_resp(uint64_t j, const lp::State &, uint64_t to, bool reject) {
    put(j, Emitted{{vs::KIND_VOTE_RESP, to, 0, 0, 0, 0, 0, reject ? 1ull : 0ull}});
  }
};
struct NoSink {
  void entry(uint64_t, uint64_t, uint64_t) {}
  void msg(uint64_t, const lp::State &, const lp::Msg &) {}
  void vote_resp(uint64_t, const lp::State &, uint64_t, bool) {}
};

static uint64_t g_hash = 0xCBF29CE484222325ull;
static void fold(uint64_t v) { g_hash = (g_hash ^ v) * 0x100000001B3ull; }

struct Brief {
  int32_t status, action;
  uint64_t n_msgs;
};

// one replay of the run, as evote_run of vote_step.hip
template <bool EMIT>
static std::vector<Brief> replay(const Case &c, uint64_t *classes) {
  lp::State s = c.s;
  vs::Vote v = c.v;
  std::vector<uint64_t> own(c.recs.size(), 0);
  vs::Run run{s.nlog};
  const bool unsupported = s.np > lp::PEERS;
  bool stopped = false;
  std::vector<Brief> out;
  for (const vs::Rec &r : c.recs) {
    vs::Out o{};
    Sink sink;
    if (stopped || unsupported) {
      o.status = stopped ? lp::ST_OK : lp::ST_UNSUPPORTED;
      o.action = stopped ? vs::NOT_STEPPED : vs::PANICKED;
      stopped = true;
    } else {
      const TermAt term_at{&c.terms, &own, run.first};
      const TypeAt type_at{&c.types, run.first};
      if (EMIT) {
        o = vs::step<true>(s, v, r, term_at, type_at, sink);
      } else {
        NoSink none;
        o = vs::step<false>(s, v, r, term_at, type_at, none);
      }
      if (o.appended) {
        run.note(s, o);
        if (o.pos - run.first >= own.size()) {
          std::printf("FAIL: a run's own entries outnumber its records\n");
          std::exit(1);
        }
        own[o.pos - run.first] = s.term;
      }
    }
    stopped = stopped || o.status != lp::ST_OK;
    out.push_back(Brief{o.status, o.action, o.n_msgs});
    if (EMIT) {
      classes[o.action]++;
      if (sink.msgs.size() != o.n_msgs || (o.appended != (sink.ent[0] != ~0ull))) {
        std::printf("FAIL: the sink got %zu messages, the record reports %llu\n", sink.msgs.size(),
                    (unsigned long long)o.n_msgs);
        std::exit(1);
      }
      fold((uint64_t)(int64_t)o.status), fold((uint64_t)o.action), fold((uint64_t)o.flags), fold(o.n_msgs);
      fold(s.term), fold(v.vote), fold(v.state);
      for (uint64_t k = 0; k < 3; ++k) fold(sink.ent[k]);
      for (const Emitted &e : sink.msgs)
        for (uint64_t k = 0; k < 8; ++k) fold(e.w[k]);
    }
  }
  if (EMIT) {
    fold(s.term), fold(s.committed), fold(s.nlog);
    for (uint32_t k = 0; k < lp::PEERS; ++k) fold(s.match[k]);
    for (uint32_t k = 0; k < lp::PEERS; ++k) fold(s.next[k]);
    fold(s.unstable), fold(s.pending);
    fold(v.state), fold(v.vote), fold(v.lead), fold(v.elapsed), fold(v.voted), fold(v.granted);
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("usage: vote_step_forms <seed> <runs>\n");
    return 2;
  }
  const uint64_t seed = std::strtoull(argv[1], nullptr, 10), runs = std::strtoull(argv[2], nullptr, 10);
  uint64_t classes[10] = {0}, records = 0;
  for (uint64_t j = 0; j < runs; ++j) {
    const Case c = draw(seed, j);
    const std::vector<Brief> a = replay<false>(c, classes), b = replay<true>(c, classes);
    records += c.recs.size();
    for (size_t k = 0; k < a.size(); ++k)
      if (a[k].status != b[k].status || a[k].action != b[k].action || a[k].n_msgs != b[k].n_msgs) {
        std::printf("FAIL: run %llu record %zu: the counting replay and the applying replay differ\n",
                    (unsigned long long)j, k);
        return 1;
      }
  }
  static const char *names[10] = {"not_stepped", "ignored", "granted", "rejected", "campaigned",
                                  "won",         "lost",    "polled",  "no_case",  "panicked"};
  std::printf("runs %llu records %llu\nclasses", (unsigned long long)runs, (unsigned long long)records);
  for (int k = 0; k < 10; ++k) std::printf(" %s=%llu", names[k], (unsigned long long)classes[k]);
  std::printf("\ndigest %llu\nok\n", (unsigned long long)g_hash);
  return 0;
}
