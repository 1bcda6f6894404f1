// conf_forms.cpp -- the host check of etcd_amd/csrc/conf_step.h: the decisions
// the kernels of conf_step.hip run, compiled for the host, over random
// requests, ConfChange bodies and gate records drawn by the generator
// tests/conf_cases.py restates draw for draw (draw_request, draw_bytes).  Every
// request is also checked against the contract's invariants: a failing request
// leaves the state as it found it, the keys stay distinct, the masks stay
// inside the slots.  The digest of every outcome is printed for the Python
// restatement to reproduce.
//
//   conf_forms <seed> <runs>
//   -> "runs N", "actions not_stepped=.. added=.. ...", "decodes ok=.. eof=.. wrong_type=.. bounds=..
//      nonterminating=..", "gates pass=.. denied=.. dropped=..", "digest H", "ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "conf_step.h"

namespace cf = conf_step;

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

static const uint64_t NP_TABLE[16] = {0, 1, 2, 3, 3, 3, 3, 4, 5, 5, 6, 6, 7, 7, 3, 8};
static const uint64_t KIND_TABLE[16] = {1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 0};
static const uint64_t NREM_TABLE[16] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 5, 5, 8, 12, 13, 13, 14};
static const uint64_t STATE_TABLE[8] = {0, 0, 0, 1, 2, 2, 0, 2};
static const uint64_t LEN_TABLE[6] = {0, 1, 3, 14, 15, 20};

struct Request {
  cf::State s;
  uint64_t kind, node;
  std::vector<uint64_t> snap;
};

static Request draw_request(SplitMix &r) {
  Request q;
  cf::State &s = q.s;
  std::memset(&s, 0, sizeof s);
  s.np = NP_TABLE[r.rnd(16)];
  uint64_t pid[cf::PEERS];
  for (uint32_t k = 0; k < cf::PEERS; ++k) pid[k] = 10 + 3 * k;
  const uint64_t idmode = r.rnd(4), ik = r.rnd(7);
  s.id = idmode == 0 ? 999 : pid[ik];
  s.term = r.rnd(5);
  s.off = r.rnd(3);
  s.nlog = r.rnd(4);
  s.pending = r.rnd(2);
  s.rstate = STATE_TABLE[r.rnd(8)];
  const uint64_t slots = s.np < cf::PEERS ? s.np : cf::PEERS;
  for (uint32_t k = 0; k < slots; ++k) {
    s.pid[k] = pid[k];
    s.match[k] = k;
    s.next[k] = k + 1;
  }
  const uint64_t mask = (1ull << slots) - 1;
  s.voted = r.next() & mask;
  s.voted &= r.next();
  s.granted = s.voted & r.next();
  s.dirty = r.rnd(2);
  s.nrem = NREM_TABLE[r.rnd(16)];
  for (uint64_t k = 0; k < s.nrem; ++k) s.rem[k] = 100 + k;
  const uint64_t remmode = r.rnd(4);
  if (s.nrem && remmode == 0) s.rem[0] = pid[2];
  if (s.nrem && remmode == 1) s.rem[0] = s.id;
  q.kind = KIND_TABLE[r.rnd(16)];
  const uint64_t nodemode = r.rnd(5), a = r.rnd(7), b = r.rnd(14);
  const uint64_t nodes[5] = {500 + a % 3, pid[0], pid[a], s.id, 100 + b};
  q.node = nodes[nodemode];
  const uint64_t ln = LEN_TABLE[r.rnd(6)], m = r.rnd(16) + 1;
  for (uint64_t k = 0; k < ln; ++k) q.snap.push_back(100 + (k % m));
  return q;
}

static std::vector<uint8_t> draw_bytes(SplitMix &r) {
  std::vector<uint8_t> out;
  const uint64_t items = r.rnd(6);
  for (uint64_t it = 0; it < items; ++it) {
    const uint64_t what = r.rnd(10);
    uint64_t v = r.next();
    v >>= r.rnd(64);
    if (what < 3) {
      out.push_back((uint8_t)((what + 1) << 3));
      while (v >= 0x80) {
        out.push_back((uint8_t)((v & 0x7F) | 0x80));
        v >>= 7;
      }
      out.push_back((uint8_t)v);
    } else if (what == 3) {
      const uint64_t ln = v % 4;
      out.push_back(0x22);
      out.push_back((uint8_t)ln);
      for (uint64_t k = 0; k < ln; ++k) out.push_back(0x61);
    } else if (what == 4) {
      out.push_back((uint8_t)((((v % 4) + 1) << 3) | (v % 4 < 3 ? 5 : 0)));
      for (int k = 0; k < 4; ++k) out.push_back(0);
    } else if (what == 5) {
      out.push_back(0x28);
      out.push_back((uint8_t)(v & 0x7F));
    } else if (what == 6) {
      out.push_back(0x29);
      for (int k = 0; k < 8; ++k) out.push_back((uint8_t)(v & 0xFF));
    } else if (what == 7) {
      const uint8_t b[4] = {0x2A, 2, 1, 2};
      out.insert(out.end(), b, b + 4);
    } else if (what == 8) {
      const uint8_t b[5] = {0x2D, 1, 2, 3, 4};
      out.insert(out.end(), b, b + 5);
    } else {
      out.push_back((v & 1) ? 0x2E : 0x2C);
    }
  }
  if (r.rnd(4) == 0 && !out.empty()) out.resize(r.rnd(out.size() + 1));
  return out;
}

// proto.Skip without groups (the generator writes none): a start-group tag ends the run
struct HostSkip {
  int32_t operator()(const uint8_t *p, int64_t l, int64_t &out) const {
    if (l <= 0) return cf::ST_PANIC_BOUNDS;
    int64_t i = 0;
    uint64_t w = 0;
    if (cf::rd_var(p, i, l, &w, 64)) return cf::ST_EOF;
    switch (w & 7) {
    case 0: {
      uint64_t v = 0;
      if (cf::rd_var(p, i, l, &v, 64)) return cf::ST_EOF;
      out = i;
      return cf::ST_OK;
    }
    case 1: out = i + 8; return cf::ST_OK;
    case 2: {
      uint64_t len = 0;
      if (cf::rd_var(p, i, l, &len, 64)) return cf::ST_EOF;
      out = (int64_t)((uint64_t)i + len);
      return cf::ST_OK;
    }
    case 3: std::printf("FAIL: the generator wrote a group\n"); std::exit(1);
    case 4: out = i; return cf::ST_OK;
    case 5: out = i + 4; return cf::ST_OK;
    default: return cf::ST_WRONG_TYPE;
    }
  }
};

struct VecAt {
  const std::vector<uint64_t> *v;
  uint64_t operator()(uint64_t j) const { return (*v)[j]; }
};

static uint64_t g_hash = 0xCBF29CE484222325ull;
static void fold(uint64_t v) { g_hash = (g_hash ^ v) * 0x100000001B3ull; }

[[noreturn]] static void fail(const char *what, uint64_t run) {
  std::printf("FAIL: run %llu: %s\n", (unsigned long long)run, what);
  std::exit(1);
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::printf("usage: conf_forms <seed> <runs>\n");
    return 2;
  }
  const uint64_t seed = std::strtoull(argv[1], nullptr, 10), runs = std::strtoull(argv[2], nullptr, 10);
  uint64_t actions[7] = {0}, decodes[5] = {0}, gates[4] = {0};
  for (uint64_t run = 0; run < runs; ++run) {
    SplitMix r(seed, run);
    const uint64_t mode = r.rnd(3);
    if (mode == 0) {
      Request q = draw_request(r);
      const cf::State s0 = q.s;
      cf::State s = q.s;
      const cf::Out o = cf::step(s, q.kind, q.node, (uint64_t)q.snap.size(), VecAt{&q.snap});
      if (o.action < cf::ADDED || o.action > cf::PANICKED) fail("no such action", run);
      if (o.status != cf::ST_OK && std::memcmp(&s, &s0, sizeof s) != 0) fail("a failing request changed the state", run);
      if ((o.status != cf::ST_OK) != (o.action == cf::PANICKED)) fail("status and action disagree", run);
      if (s.np <= cf::PEERS) {
        for (uint32_t j = 0; j < s.np; ++j)
          for (uint32_t k = 0; k < j; ++k)
            if (s.pid[j] == s.pid[k]) fail("two equal keys in prs", run);
        if ((s.voted | s.granted) >> s.np) fail("a vote outside the slots", run);
      }
      if (s.nrem > cf::REMOVED) fail("more removed ids than the record holds", run);
      for (uint32_t j = 0; j < s.nrem; ++j)
        for (uint32_t k = 0; k < j; ++k)
          if (s.rem[j] == s.rem[k]) fail("an id stored twice in removed", run);
      if (o.n_msgs > 1 || (o.n_msgs && o.action != cf::DENIED_BACK)) fail("a message from the wrong action", run);
      actions[o.action]++;
      fold((uint64_t)(int64_t)o.status), fold((uint64_t)o.action), fold(o.n_msgs), fold(s.np);
      for (uint32_t k = 0; k < cf::PEERS; ++k) fold(s.pid[k]);
      for (uint32_t k = 0; k < cf::PEERS; ++k) fold(s.match[k]);
      for (uint32_t k = 0; k < cf::PEERS; ++k) fold(s.next[k]);
      fold(s.pending), fold(s.voted), fold(s.granted), fold(s.dirty), fold(s.nrem);
      for (uint32_t k = 0; k < cf::REMOVED; ++k) fold(s.rem[k]);
    } else if (mode == 1) {
      const std::vector<uint8_t> b = draw_bytes(r);
      // an exact-size copy: a read past the body is the sanitizer's to see
      uint8_t *p = (uint8_t *)std::malloc(b.size() ? b.size() : 1);
      if (!b.empty()) std::memcpy(p, b.data(), b.size());
      cf::ConfChange cc;
      const int32_t st = cf::decode(p, (int64_t)b.size(), HostSkip{}, &cc);
      std::free(p);
      const int slot = st == cf::ST_OK ? 0 : st == cf::ST_EOF ? 1 : st == cf::ST_WRONG_TYPE ? 2
                       : st == cf::ST_PANIC_BOUNDS ? 3 : st == cf::ST_NONTERMINATING ? 4 : -1;
      if (slot < 0) fail("no such decode status", run);
      decodes[slot]++;
      fold((uint64_t)(int64_t)st), fold(cc.id), fold((uint64_t)(uint32_t)cc.type), fold(cc.node);
    } else {
      const Request q = draw_request(r);
      uint64_t w[1 + cf::REMOVED];
      w[0] = q.s.nrem;
      for (uint32_t k = 0; k < cf::REMOVED; ++k) w[1 + k] = q.s.rem[k];
      const int32_t action = cf::gate(w, q.s.id, q.node);
      if (action < cf::G_PASS || action > cf::G_DROPPED) fail("no such gate action", run);
      if ((action == cf::G_PASS) == cf::is_removed(q.s, q.node)) fail("the gate and removed[] disagree", run);
      gates[action]++;
      fold((uint64_t)action);
    }
  }
  static const char *names[7] = {"not_stepped", "added", "removed", "denied_back", "stopped", "reloaded", "panicked"};
  std::printf("runs %llu\nactions", (unsigned long long)runs);
  for (int k = 0; k < 7; ++k) std::printf(" %s=%llu", names[k], (unsigned long long)actions[k]);
  std::printf("\ndecodes ok=%llu eof=%llu wrong_type=%llu bounds=%llu nonterminating=%llu\n",
              (unsigned long long)decodes[0], (unsigned long long)decodes[1], (unsigned long long)decodes[2],
              (unsigned long long)decodes[3], (unsigned long long)decodes[4]);
  std::printf("gates pass=%llu denied=%llu dropped=%llu\ndigest %llu\nok\n", (unsigned long long)gates[1],
              (unsigned long long)gates[2], (unsigned long long)gates[3], (unsigned long long)g_hash);
  return 0;
}
