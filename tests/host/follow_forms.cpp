// follow_forms.cpp -- the host check of etcd_amd/csrc/follow_step.h: the serial
// follower step the kernels of follow_step.hip run, compiled for the host, over
// random runs drawn by the generator tests/follow_cases.py restates draw for
// draw (draw).  Every run is replayed twice, as the kernels do -- the counting
// pass, then the applying pass -- on the log as the call found it, the run's
// own suffix seen through the overlay only; the two replays must agree.  Then
// the copy is done as the copy pass does it, and the digest of every outcome,
// response, final record and final log is printed for the Python restatement
// (which keeps a real list of entries and no overlay) to reproduce.
//
//   follow_forms <seed> <runs>
//   -> "runs N records M", "classes not_stepped=.. ... panicked=..", "statuses ok=.. ...", "digest H", "ok"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "follow_step.h"

namespace fs = follow_step;
namespace lp = lead_prop;
namespace vs = vote_step;

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

static const uint64_t NP_TABLE[16] = {1, 2, 3, 3, 3, 3, 5, 5, 7, 3, 2, 3, 3, 5, 0, 8};
static const uint64_t OFF_TABLE[6] = {0, 0, 5, 1000, ~0ull - 7, 0};
static const uint64_t STATE_TABLE[8] = {0, 0, 0, 0, 1, 1, 2, 0};
static const uint64_t NE_TABLE[8] = {0, 0, 0, 1, 1, 2, 3, 5};
static const uint64_t NN_TABLE[8] = {1, 2, 3, 3, 5, 9, 9, 65};
static const uint64_t RG_TABLE[8] = {40, 40, 40, 3, 40, 40, 6, 40};

struct Msg {
  fs::Rec r;
  fs::Snap sn;
  uint64_t src_first;              // Entries in Case::src
  std::vector<uint64_t> nodes;
};

struct Case {
  lp::State s;
  vs::Vote v;
  fs::Ready rd;
  std::vector<uint64_t> terms, src;
  std::vector<Msg> msgs;
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
  }
  s.term = t + r.rnd(2);
  s.committed = s.off + (r.rnd(2) ? r.rnd(s.nlog + 1) : 0);
  for (uint64_t k = 0; k < slots; ++k) s.pid[k] = 10 + 3 * k + r.rnd(3);
  const uint64_t me = slots ? r.rnd(slots) : 0;
  s.id = slots ? s.pid[me] : 10;
  if (r.rnd(5) == 0) s.id = 999;
  for (uint64_t k = 0; k < slots; ++k) {
    s.match[k] = s.off + r.rnd(s.nlog + 1);
    s.next[k] = s.match[k] + 1;
  }
  c.v.state = STATE_TABLE[r.rnd(8)];
  c.v.vote = r.rnd(2) * 77;
  c.v.lead = r.rnd(2) * s.id;
  c.v.elapsed = r.rnd(10);
  c.v.voted = c.v.granted = 0;
  if (c.v.state == vs::CANDIDATE) {
    c.v.voted = r.next() & ((1ull << slots) - 1);
    c.v.granted = c.v.voted & r.next();
  } else if (r.rnd(16) == 0 && slots) {
    c.v.voted = 1;
  }
  s.unstable = s.off + r.rnd(s.nlog + 3);
  s.pending = r.rnd(2);
  c.rd.applied = r.rnd(4);
  c.rd.soft_dirty = r.rnd(2);
  s.efirst = 0;
  s.fresh = s.nlog;
  s.snap_ok = false;
  uint64_t cur = s.term;
  const uint64_t nrec = 1 + r.rnd(5);
  for (uint64_t j = 0; j < nrec; ++j) {
    Msg m;
    m.r = fs::Rec{};
    m.sn = fs::Snap{0, 0, 0};
    m.src_first = c.src.size();
    m.r.kind = r.rnd(4) == 0 ? fs::KIND_SNAP : fs::KIND_APP;
    m.r.from = 55;
    if (slots) {
      if (r.rnd(8)) m.r.from = s.pid[r.rnd(slots)];
    }
    const uint64_t rel = r.rnd(8);
    m.r.term = rel == 0 ? 0 : rel == 1 ? cur - 1 : rel == 7 ? cur + 2 : cur + (r.rnd(4) == 0 ? 1 : 0);
    cur = m.r.term > cur ? m.r.term : cur;
    if (m.r.kind == fs::KIND_APP) {
      m.r.index = s.off + r.rnd(s.nlog + 2);
      const uint64_t pos = m.r.index - s.off;
      const uint64_t mode = r.rnd(4);
      m.r.log_term = (mode != 0 && pos < s.nlog) ? c.terms[pos] : r.rnd(t + 2);
      m.r.n_ents = NE_TABLE[r.rnd(8)];
      for (uint64_t k = 0; k < m.r.n_ents; ++k) {
        const uint64_t p = pos + 1 + k;
        c.src.push_back((p < s.nlog && r.rnd(4)) ? c.terms[p] : t + r.rnd(2));
      }
      m.r.commit = s.off + r.rnd(s.nlog + 4);
    } else {
      m.sn.index = s.committed + r.rnd(4) - 1;
      m.sn.term = 1 + r.rnd(5);
      const uint64_t j8 = r.rnd(8);
      m.sn.n_nodes = NN_TABLE[j8];
      for (uint64_t k = 0; k < m.sn.n_nodes; ++k) m.nodes.push_back(r.rnd(4) == 0 ? s.id : 10 + r.rnd(RG_TABLE[j8]));
    }
    c.msgs.push_back(m);
  }
  return c;
}

static uint64_t g_hash = 0xCBF29CE484222325ull;
static void fold(uint64_t v) { g_hash = (g_hash ^ v) * 0x100000001B3ull; }

struct Final {
  lp::State s;
  vs::Vote v;
  fs::Ready rd;
  fs::Overlay ov;
};

// one replay of the run, as efollow_run of follow_step.hip
static std::vector<fs::Out> replay(const Case &c, Final *fin, std::vector<uint64_t> *terms_after) {
  lp::State s = c.s;
  vs::Vote v = c.v;
  fs::Ready rd = c.rd;
  fs::Run run = fs::run_start();
  std::vector<fs::Out> out;
  for (const Msg &m : c.msgs) {
    const fs::Overlay ov = run.ov;
    const auto log_at = [&](uint64_t pos) { return c.terms.at(pos); };
    const auto src_at = [&](uint64_t q) { return c.src.at(q); };
    const auto term_at = [&](uint64_t pos) { return fs::overlay_term(ov, pos, log_at, src_at); };
    const auto src_term = [&](uint64_t k) { return c.src.at(m.src_first + k); };
    const auto node_at = [&](uint64_t k) { return m.nodes.at(k); };
    fs::Out o = fs::run_step(run, s, v, rd, m.r, m.src_first, m.sn, term_at, src_term, node_at);
    out.push_back(o);
    if (terms_after) {
      fold((uint64_t)(int64_t)o.status), fold((uint64_t)o.action), fold((uint64_t)o.flags), fold(o.n_msgs);
      fold(o.conflict), fold(o.n_app), fold(o.n_app ? o.dst_pos : 0), fold(s.nlog - 1 + s.off), fold(s.committed);
      fold(s.term), fold(v.state);
    }
  }
  if (terms_after) {
    // the responses, after the run's outcomes (the restatement's order)
    lp::State s2 = c.s;
    vs::Vote v2 = c.v;
    fs::Ready rd2 = c.rd;
    fs::Run run2 = fs::run_start();
    for (const Msg &m : c.msgs) {
      const fs::Overlay ov = run2.ov;
      const auto log_at = [&](uint64_t pos) { return c.terms.at(pos); };
      const auto src_at = [&](uint64_t q) { return c.src.at(q); };
      const auto term_at = [&](uint64_t pos) { return fs::overlay_term(ov, pos, log_at, src_at); };
      const auto src_term = [&](uint64_t k) { return c.src.at(m.src_first + k); };
      const auto node_at = [&](uint64_t k) { return m.nodes.at(k); };
      const fs::Out o = fs::run_step(run2, s2, v2, rd2, m.r, m.src_first, m.sn, term_at, src_term, node_at);
      if (o.n_msgs) fold(m.r.from), fold(s2.id), fold(s2.term), fold(o.resp_index), fold(o.resp_reject ? 1 : 0);
    }
    // the copy pass
    *terms_after = c.terms;
    if (run.ov.restored) {
      terms_after->assign(1, run.ov.term);
    } else if (run.ov.n) {
      terms_after->resize(run.ov.pos);
      for (uint64_t k = 0; k < run.ov.n; ++k) terms_after->push_back(c.src.at(run.ov.src + k));
    }
    if (terms_after->size() != s.nlog && s.np <= lp::PEERS) {
      std::printf("FAIL: the log holds %zu entries, the record says %llu\n", terms_after->size(),
                  (unsigned long long)s.nlog);
      std::exit(1);
    }
  }
  fin->s = s;
  fin->v = v;
  fin->rd = rd;
  fin->ov = run.ov;
  return out;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("usage: follow_forms <seed> <runs>\n");
    return 2;
  }
  const uint64_t seed = std::strtoull(argv[1], nullptr, 10), runs = std::strtoull(argv[2], nullptr, 10);
  uint64_t classes[9] = {0}, statuses[4] = {0}, records = 0;
  for (uint64_t j = 0; j < runs; ++j) {
    const Case c = draw(seed, j);
    Final fa, fb;
    std::vector<uint64_t> terms;
    const std::vector<fs::Out> a = replay(c, &fa, nullptr), b = replay(c, &fb, &terms);
    records += c.msgs.size();
    for (size_t k = 0; k < a.size(); ++k) {
      if (a[k].status != b[k].status || a[k].action != b[k].action || a[k].n_msgs != b[k].n_msgs ||
          a[k].n_app != b[k].n_app) {
        std::printf("FAIL: run %llu record %zu: the counting replay and the applying replay differ\n",
                    (unsigned long long)j, k);
        return 1;
      }
      classes[b[k].action]++;
      statuses[b[k].status == 0 ? 0 : b[k].status == 33 ? 1 : b[k].status == 38 ? 2 : 3]++;
    }
    const lp::State &s = fb.s;
    fold(s.term), fold(s.committed), fold(s.off), fold(s.nlog), fold(s.np);
    for (uint32_t k = 0; k < lp::PEERS; ++k) fold(s.pid[k]);
    for (uint32_t k = 0; k < lp::PEERS; ++k) fold(s.match[k]);
    for (uint32_t k = 0; k < lp::PEERS; ++k) fold(s.next[k]);
    fold(s.unstable), fold(s.pending);
    fold(fb.v.state), fold(fb.v.vote), fold(fb.v.lead), fold(fb.v.elapsed), fold(fb.v.voted), fold(fb.v.granted);
    fold(fb.rd.applied), fold(fb.rd.soft_dirty);
    for (uint64_t t : terms) fold(t);
  }
  static const char *names[9] = {"not_stepped", "ignored",    "no_case",  "appended", "rejected",
                                 "restored",    "snap_stale", "deferred", "panicked"};
  static const char *snames[4] = {"ok", "bounds", "committed_conflict", "unsupported"};
  std::printf("runs %llu records %llu\nclasses", (unsigned long long)runs, (unsigned long long)records);
  for (int k = 0; k < 9; ++k) std::printf(" %s=%llu", names[k], (unsigned long long)classes[k]);
  std::printf("\nstatuses");
  for (int k = 0; k < 4; ++k) std::printf(" %s=%llu", snames[k], (unsigned long long)statuses[k]);
  std::printf("\ndigest %llu\nok\n", (unsigned long long)g_hash);
  return 0;
}
