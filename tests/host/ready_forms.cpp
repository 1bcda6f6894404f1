// ready_forms.cpp -- the host check of etcd_amd/csrc/ready_step.h: the
// per-group decision the kernels of ready_step.hip run (newReady, the record
// count of Save, what accepting leaves) and their record conversion, compiled
// for the host, over random groups drawn by the generator
// tests/ready_cases.py restates draw for draw (random_group).  The digest of
// every outcome and save record is printed for the Python restatement to
// reproduce.
//
//   ready_forms <seed> <groups>
//   -> "groups N records M", "classes void=.. ... committed_nil=..", "digest H", "ok"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ready_step.h"

namespace rs = ready_step;
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

static const uint64_t OFF_TABLE[8] = {0, 0, 0, 5, 1000, 1000, ~0ull - 1, 7};

struct Entry {
  uint64_t w[5];                                     // term, index, data_off, data_len, type | data_nil << 32
};

struct Case {
  rs::In in;
  std::vector<Entry> log;
};

static Case draw(uint64_t seed, uint64_t j) {
  SplitMix r(seed, j);
  Case c;
  rs::In &g = c.in;
  g.off = OFF_TABLE[r.rnd(8)];
  g.nlog = r.rnd(7);
  uint64_t data_off = 0;
  for (uint64_t k = 0; k < g.nlog; ++k) {
    const uint64_t etype = r.rnd(4) == 0 ? 1 : 0;
    const uint64_t data_len = r.rnd(3) ? r.rnd(100) : 0;
    uint64_t data_nil = data_len == 0 ? r.rnd(2) : 0;
    if (r.rnd(40) == 0) data_nil = 2;
    const uint64_t term = 1 + r.rnd(3);
    c.log.push_back(Entry{{term, g.off + k, data_off, data_len, etype | (data_nil << 32)}});
    data_off += data_len;
  }
  const uint64_t end = g.off + g.nlog;
  uint64_t rel = r.rnd(6);
  const uint64_t u2 = g.off + r.rnd(g.nlog + 1), u3 = g.off + r.rnd(g.nlog + 2);
  const uint64_t unstable_of[6] = {end, end, u2, u3, 0, g.off - 1};
  g.unstable = unstable_of[rel];
  g.committed = g.off + r.rnd(g.nlog + 2);
  rel = r.rnd(4);
  const uint64_t a1 = g.off + r.rnd(g.committed - g.off + 1);
  const uint64_t applied_of[4] = {g.committed, a1, g.committed - 1, g.off};
  g.applied = applied_of[rel];
  g.term = 1 + r.rnd(5);
  g.vote = r.rnd(3);
  g.lead = r.rnd(3);
  g.state = r.rnd(3);
  if (r.rnd(3) == 0) {
    g.hs_term = g.term;
    g.hs_vote = g.vote;
    g.hs_commit = g.committed;
  } else {
    g.hs_term = g.term - r.rnd(2);
    g.hs_vote = g.vote;
    g.hs_commit = g.committed - r.rnd(2);
  }
  g.plead = g.lead;
  if (!r.rnd(2)) g.plead = r.rnd(3);
  g.pstate = g.state;
  if (!r.rnd(2)) g.pstate = r.rnd(3);
  g.soft_dirty = r.rnd(8) == 0 ? 1 : 0;
  g.snap_index = r.rnd(3) == 0 ? (g.off ? g.off : 3) : 0;
  g.snapi = g.snap_index;
  if (!r.rnd(2)) g.snapi = r.rnd(3);
  return c;
}

static uint64_t g_hash = 0xCBF29CE484222325ull;
static void fold(uint64_t v) { g_hash = (g_hash ^ v) * 0x100000001B3ull; }

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("usage: ready_forms <seed> <groups>\n");
    return 2;
  }
  const uint64_t seed = std::strtoull(argv[1], nullptr, 10), groups = std::strtoull(argv[2], nullptr, 10);
  uint64_t classes[9] = {0}, records = 0;
  for (uint64_t j = 0; j < groups; ++j) {
    const Case c = draw(seed, j);
    rs::Out o = rs::decide(c.in);
    if (o.status == lp::ST_OK) {
      if (o.ents_pos + o.n_ents > c.log.size() || o.committed_pos + o.n_committed > c.log.size()) {
        std::printf("FAIL: group %llu: a view leaves the log\n", (unsigned long long)j);
        return 1;
      }
      // as k_ready_count: an unstable entry whose Data is outside d_data
      for (uint64_t k = 0; k < o.n_ents; ++k)
        if (rs::data_outside((int32_t)(c.log[o.ents_pos + k].w[4] >> 32))) o.status = lp::ST_UNSUPPORTED;
    }
    if (o.status != lp::ST_OK) {                     // the status alone
      rs::Out v{};
      v.status = o.status;
      v.applied = c.in.applied;
      v.unstable = c.in.unstable;
      o = v;
    }
    if (o.status != lp::ST_OK) {
      classes[0]++;
    } else {
      classes[1] += (o.flags & rs::SOFT) ? 1 : 0;
      classes[2] += (o.flags & rs::HARD) ? 1 : 0;
      classes[3] += (o.flags & rs::SNAP) ? 1 : 0;
      classes[4] += (o.flags & rs::UPDATES) ? 1 : 0;
      classes[5] += o.n_ents ? 1 : 0;
      classes[6] += o.n_ents ? 0 : 1;
      classes[7] += o.n_committed ? 1 : 0;
      classes[8] += o.n_committed ? 0 : 1;
    }
    fold((uint64_t)(uint32_t)o.status), fold((uint64_t)(uint32_t)o.flags), fold(o.term), fold(o.vote), fold(o.commit);
    fold(o.ents_pos), fold(o.n_ents), fold(o.committed_pos), fold(o.n_committed), fold(o.n_save), fold(o.lead);
    fold(o.state), fold(o.applied), fold(o.unstable);
    // Save's records, as k_ready_emit builds them
    uint64_t made = 0;
    if (o.status == lp::ST_OK) {
      uint64_t w[7];
      if (o.flags & rs::HARD) {
        rs::save_of_state(w, c.in.term, c.in.vote, c.in.committed);
        for (int k = 0; k < 7; ++k) fold(w[k]);
        ++made;
      }
      for (uint64_t k = 0; k < o.n_ents; ++k) {
        rs::save_of_entry(w, c.log[o.ents_pos + k].w);
        for (int q = 0; q < 7; ++q) fold(w[q]);
        ++made;
      }
    }
    if (made != o.n_save) {
      std::printf("FAIL: group %llu: %llu records made, n_save %llu\n", (unsigned long long)j, (unsigned long long)made,
                  (unsigned long long)o.n_save);
      return 1;
    }
    records += made;
  }
  static const char *names[9] = {"void", "soft", "hard", "snap", "updates", "ents", "ents_nil", "committed",
                                 "committed_nil"};
  std::printf("groups %llu records %llu\nclasses", (unsigned long long)groups, (unsigned long long)records);
  for (int k = 0; k < 9; ++k) std::printf(" %s=%llu", names[k], (unsigned long long)classes[k]);
  std::printf("\ndigest %llu\nok\n", (unsigned long long)g_hash);
  return 0;
}
