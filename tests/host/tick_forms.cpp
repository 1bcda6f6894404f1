// tick_forms.cpp -- the host check of etcd_amd/csrc/tick_step.h: the decision
// the kernels of tick_step.hip run, compiled for the host, over random ticks
// drawn by the generator tests/tick_cases.py restates draw for draw
// (draw_case).  Every tick that reaches isElectionTimeout's last line is also
// decided by the plain form -- d > r % election as Go writes it -- against the
// shortcut the kernels take (d >= election fires without the modulo), at its
// own draw and at the draw's edges; a difference fails the run.  The digest of
// every outcome is printed for the Python restatement to reproduce.
//
//   tick_forms <seed> <runs>
//   -> "runs N", "actions idle=.. held=.. hup=.. beat=.. not_promotable=.. panicked=..",
//      "forms shortcut=.. modulo=..", "pins ok", "digest H", "ok"
#include <cstdio>
#include <cstdlib>

#include "tick_step.h"

namespace ts = tick_step;

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

static const uint64_t INT_MAX31 = 0x7fffffffull, M63 = 0x7fffffffffffffffull;
static const uint64_t ELECTION_TABLE[6] = {1, 2, 10, 10, 10, INT_MAX31};
static const uint64_t HEARTBEAT_TABLE[4] = {0, 1, 1, 5};
static const uint64_t STATE_TABLE[6] = {0, 0, 0, 1, 2, 2};
static const uint64_t NP_TABLE[8] = {0, 1, 3, 3, 3, 5, 7, 8};

struct Case {
  ts::In in;
  uint64_t election, heartbeat, val;
  bool have_draw;
};

static Case draw(uint64_t seed, uint64_t run) {
  SplitMix r(seed, run);
  Case c;
  c.election = ELECTION_TABLE[r.rnd(6)];
  c.heartbeat = HEARTBEAT_TABLE[r.rnd(4)];
  c.in.state = STATE_TABLE[r.rnd(6)];
  c.in.np = NP_TABLE[r.rnd(8)];
  for (uint32_t k = 0; k < ts::PEERS; ++k) c.in.pid[k] = 10 + 3 * k;
  const uint64_t idmode = r.rnd(6), k = r.rnd(7);
  c.in.id = idmode == 0 ? 999 : idmode == 1 ? c.in.pid[0] : c.in.pid[k];
  c.in.term = r.rnd(5);
  const uint64_t emode = r.rnd(10), x = r.rnd(2), y = r.next(), e = c.election;
  const uint64_t table[10] = {0,   e - 2,      e - 1,     e, 2 * e - 2, 2 * e - 1,
                              M63, x ? ~0ull : M63 + 1, e - 1 + y % e, c.heartbeat - 1 + y % 3};
  c.in.elapsed = table[emode];
  c.have_draw = r.rnd(2) != 0;
  const uint64_t dmode = r.rnd(5), z = r.next();
  const uint64_t dtable[5] = {0, e - 1, e, M63, z >> 1};
  c.val = c.have_draw ? dtable[dmode] : z;
  return c;
}

static uint64_t g_hash = 0xCBF29CE484222325ull;
static void fold(uint64_t v) { g_hash = (g_hash ^ v) * 0x100000001B3ull; }

[[noreturn]] static void fail(const char *what, uint64_t run) {
  std::printf("FAIL: run %llu: %s\n", (unsigned long long)run, what);
  std::exit(1);
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("usage: tick_forms <seed> <runs>\n");
    return 2;
  }
  const uint64_t seed = std::strtoull(argv[1], nullptr, 10), runs = std::strtoull(argv[2], nullptr, 10);
  uint64_t actions[7] = {0}, forms[2] = {0};
  for (uint64_t run = 0; run < runs; ++run) {
    const Case c = draw(seed, run);
    const ts::Out o = ts::decide(c.in, (int64_t)c.election, (int64_t)c.heartbeat, c.have_draw, c.val);
    if (o.action < ts::IDLE || o.action > ts::PANICKED) fail("no such action", run);
    actions[o.action]++;
    if (o.action == ts::HUP || o.action == ts::HELD) {
      const int64_t d = (int64_t)(c.in.elapsed + 1 - c.election), el = (int64_t)c.election;
      if (d < 0) fail("a draw was consumed below the election timeout", run);
      forms[d >= el ? 0 : 1]++;
      const uint64_t rs[6] = {o.draw, 0, c.election - 1, c.election, M63, (uint64_t)d};
      for (uint64_t rr : rs)
        if (ts::fires(d, rr & M63, el) != ts::fires_plain(d, rr & M63, el)) fail("the shortcut differs from the plain form", run);
      if ((o.action == ts::HUP) != ts::fires_plain(d, o.draw, el)) fail("the action is not the plain form's", run);
      if (!c.have_draw && o.draw != ts::draw(c.val, c.in.id, c.in.term, c.in.elapsed + 1)) fail("the draw", run);
    } else if (o.draw != 0) {
      fail("a draw reported where none is consumed", run);
    }
    fold((uint64_t)(int64_t)o.status), fold((uint64_t)o.action), fold(o.elapsed), fold(o.draw);
  }
  if (ts::draw(0, 0, 0, 0) != 0 || ts::draw(1, 2, 3, 4) != 0x5a86a12931d3dfc7ull ||
      ts::draw(~0ull, ~0ull, ~0ull, ~0ull) != 0x343596642af3c78eull)
    fail("etick_draw's pins", 0);
  static const char *names[7] = {"", "idle", "held", "hup", "beat", "not_promotable", "panicked"};
  std::printf("runs %llu\nactions", (unsigned long long)runs);
  for (int k = 1; k < 7; ++k) std::printf(" %s=%llu", names[k], (unsigned long long)actions[k]);
  std::printf("\nforms shortcut=%llu modulo=%llu\npins ok\ndigest %llu\nok\n", (unsigned long long)forms[0],
              (unsigned long long)forms[1], (unsigned long long)g_hash);
  return 0;
}
