// node_forms.cpp -- the host check of etcd_amd/csrc/node_start.h: the decisions
// the kernels of node_start.hip run, compiled for the host, over random
// requests drawn by the generator tests/node_cases.py restates draw for draw
// (draw_case).  Every built node is also checked against what Go's code says
// directly: a fresh raft's zeros, loadState without a clamp, loadEnts' unstable,
// the seeding of a StartNode, and that a request which is not built says
// nothing else.  The digest of every outcome is printed for the Python
// restatement to reproduce.
//
//   node_forms <seed> <runs>
//   -> "runs N", "actions none=.. restarted=.. restarted_snap=.. started=.. panicked=..",
//      "digest H", "ok"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "node_start.h"

namespace ns = node_start;

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

static const uint64_t KIND_TABLE[8] = {1, 1, 1, 1, 2, 2, 2, 0};
static const uint64_t ID_TABLE[8] = {0, 1, 2, 3, 127, 128, 1ull << 56, 1ull << 63};
static const uint64_t NSRC_TABLE[6] = {0, 1, 2, 3, 5, 9};
static const uint64_t INDEX_TABLE[6] = {0, 1, 5, 100, ~0ull, 1ull << 40};
static const uint64_t NN_TABLE[8] = {0, 1, 3, 3, 7, 12, 64, 65};
static const uint64_t POOL_TABLE[4] = {3, 7, 8, 20};
static const uint64_t NR_TABLE[6] = {0, 1, 3, 14, 15, 20};
static const uint64_t RPOOL_TABLE[4] = {3, 14, 15, 30};
static const uint64_t CLEN_TABLE[4] = {0, 1, 127, 128};

struct Peer {
  uint64_t id, clen;
};

struct Case {
  ns::Req req;
  ns::Snap snap;
  std::vector<uint64_t> nodes, removed;
  std::vector<Peer> peers;
};

static Case draw(uint64_t seed, uint64_t run) {
  SplitMix r(seed, run);
  Case c;
  c.req.kind = KIND_TABLE[r.rnd(8)];
  c.req.id = ID_TABLE[r.rnd(8)];
  c.req.n_src = NSRC_TABLE[r.rnd(6)];
  c.req.hs_term = r.rnd(5);
  c.req.hs_vote = r.rnd(4);
  const uint64_t cmode = r.rnd(4);
  c.req.has_snap = r.rnd(3) != 0;
  c.snap.index = INDEX_TABLE[r.rnd(6)];
  c.snap.term = r.rnd(7);
  const uint64_t any = r.rnd(200);
  const uint64_t commits[4] = {0, c.snap.index - 1, c.snap.index + 1, any};
  c.req.hs_commit = commits[cmode];
  const uint64_t nn = NN_TABLE[r.rnd(8)], pool = POOL_TABLE[r.rnd(4)];
  for (uint64_t j = 0; j < nn; ++j) c.nodes.push_back(1 + r.rnd(pool));
  const uint64_t nr = NR_TABLE[r.rnd(6)], rpool = RPOOL_TABLE[r.rnd(4)];
  for (uint64_t j = 0; j < nr; ++j) c.removed.push_back(1 + r.rnd(rpool));
  for (uint64_t j = 0; j < c.req.n_src; ++j) {
    const uint64_t id = ID_TABLE[r.rnd(8)];
    c.peers.push_back(Peer{id, CLEN_TABLE[r.rnd(4)]});
  }
  c.snap.n_nodes = nn;
  c.snap.n_removed = nr;
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
    std::printf("usage: node_forms <seed> <runs>\n");
    return 2;
  }
  const uint64_t seed = std::strtoull(argv[1], nullptr, 10), runs = std::strtoull(argv[2], nullptr, 10);
  uint64_t actions[5] = {0};
  for (uint64_t run = 0; run < runs; ++run) {
    const Case c = draw(seed, run);
    ns::Node n = ns::Node();                         // build() leaves it alone where nothing is built
    const auto node_at = [&](uint64_t j) { return c.nodes.at(j); };
    const auto rem_at = [&](uint64_t j) { return c.removed.at(j); };
    const ns::Out o = ns::build(n, c.req, c.snap, node_at, rem_at);
    if (o.action < ns::NONE || o.action > ns::PANICKED) fail("no such action", run);
    actions[o.action]++;
    fold((uint64_t)(int64_t)o.status), fold((uint64_t)o.action);
    if ((o.action == ns::PANICKED) != (o.status != ns::ST_OK)) fail("status and action disagree", run);
    if ((c.req.kind == ns::KIND_NONE) != (o.action == ns::NONE)) fail("kind 0 and ENODE_NONE disagree", run);
    if (c.req.kind != ns::KIND_NONE && c.req.id == 0 && o.status != ns::ST_PANIC_NONE_ID) fail("the none id", run);
    if (o.status != ns::ST_OK || o.action == ns::NONE) continue;
    uint64_t g[32], p[4], v[8], r[8], cw[16];
    ns::words(n, run, c.req.n_src + 1, g, p, v, r, cw);
    // newRaft and becomeFollower(0, None): what neither constructor touches
    for (int k = 0; k < 8; ++k)
      if (v[k] != (k == 1 ? n.vote : 0)) fail("the evote_state of a fresh follower", run);
    if (p[2] != 0 || r[3] != 0 || r[4] != 0 || r[7] != 0) fail("pending_conf, the previous SoftState, soft_dirty", run);
    if (n.np > ns::PEERS || n.nrem > ns::REMOVED) fail("more slots than the records have", run);
    for (uint32_t k = 0; k < ns::PEERS; ++k)
      if (k >= n.np && (n.pid[k] | n.match[k] | n.next[k])) fail("a slot past n_peers", run);
    if (c.req.kind == ns::KIND_START) {
      if (o.action != ns::STARTED || n.nlog != 1 + c.req.n_src || n.committed != c.req.n_src || n.unstable != 0 ||
          n.np != 0 || n.nrem != 0 || n.term != 0 || n.off != 0 || n.applied != 0 || n.restored)
        fail("StartNode's log", run);
      if (r[0] != 0 || r[1] != 0 || r[2] != c.req.n_src || r[5] != 0) fail("StartNode's seeding", run);
    } else {
      const bool restored = c.req.has_snap && c.snap.index > 0;
      if (n.restored != restored || (o.action == ns::RESTARTED_SNAP) != restored) fail("restore's return value", run);
      if (n.term != c.req.hs_term || n.vote != c.req.hs_vote || n.committed != c.req.hs_commit) fail("loadState", run);
      if (r[0] != c.req.hs_term || r[1] != c.req.hs_vote || r[2] != c.req.hs_commit) fail("prevHardSt", run);
      const uint64_t off = restored ? c.snap.index : 0;
      if (n.off != off || n.applied != off || n.snapi != off) fail("raftLog.restore", run);
      if (n.nlog != c.req.n_src || n.unstable != off + c.req.n_src) fail("loadEnts", run);
      if (!restored && (n.np != 0 || n.nrem != 0)) fail("a snapshot that was not taken left something", run);
      for (uint32_t k = 0; k < ns::PEERS && k < n.np; ++k)
        if (n.next[k] != off + 1 || n.match[k] != (n.pid[k] == n.id ? off : 0)) fail("restore's progress", run);
    }
    for (int k = 0; k < 32; ++k) fold(g[k]);
    for (int k = 0; k < 4; ++k) fold(p[k]);
    for (int k = 0; k < 8; ++k) fold(v[k]);
    for (int k = 0; k < 8; ++k) fold(r[k]);
    for (int k = 0; k < 16; ++k) fold(cw[k]);
    fold(n.restored ? 1 : 0);
    if (c.req.kind == ns::KIND_START)
      for (const Peer &pe : c.peers) {
        uint8_t head[ns::CONF_HEAD_MAX];
        const uint64_t hl = (uint64_t)(ns::conf_change_head(head, pe.id, pe.clen) - head);
        if (hl > ns::CONF_HEAD_MAX || hl + pe.clen != ns::conf_change_size(pe.id, pe.clen)) fail("the ConfChange's size", run);
        fold(hl + pe.clen);
        for (uint64_t b = 0; b < hl; ++b) fold(head[b]);
      }
  }
  static const char *names[5] = {"none", "restarted", "restarted_snap", "started", "panicked"};
  std::printf("runs %llu\nactions", (unsigned long long)runs);
  for (int k = 0; k < 5; ++k) std::printf(" %s=%llu", names[k], (unsigned long long)actions[k]);
  std::printf("\ndigest %llu\nok\n", (unsigned long long)g_hash);
  return 0;
}
