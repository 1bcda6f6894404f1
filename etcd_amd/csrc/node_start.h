// node_start.h -- the decisions of the batched StartNode / RestartNode
// (enode_batch_device), shared by its kernels (node_start.hip) and the host
// check (tests/host/node_forms.cpp).  Plain C++17, no HIP header.
//
// build() is raft.StartNode or raft.RestartNode (raft/node.go:125-161) on one
// request: newRaft(id, nil, ...) with newLog and becomeFollower(0, None)
// (raft/raft.go:135-154, raft/log.go:26-34), raft.restore (raft.go:535-554 with
// raftLog.restore, log.go:185-192), loadState and loadEnts (raft.go:597-606,
// log.go:40-43), StartNode's append and commit (node.go:141-142) and the
// locals node.run starts with (node.go:194-197).  It moves no entry and writes
// no byte: it says what the five records of the group hold afterwards.
// words() is their layout; conf_change_size() / conf_change_head() are
// ConfChange{ID 0, Type 0, NodeID, Context}.Marshal() (raft/raftpb/raft.pb.go:
// 1108-1130) with ewal_wire.h's varints.  All arithmetic is Go's uint64 and
// wraps.
#pragma once
#include "ewal_wire.h"

#ifdef __HIPCC__
#define NS_UNROLL _Pragma("unroll")
#else
#define NS_UNROLL
#endif

namespace node_start {

constexpr uint32_t PEERS = 7, REMOVED = 14;
constexpr uint64_t MAX_NODES = 64;                   // the longest Snapshot.Nodes a restore reads
constexpr uint64_t NO_SNAP = ~0ull;                  // enode_req.snap: snapshot == nil
constexpr int32_t ST_OK = 0, ST_UNSUPPORTED = 48, ST_PANIC_NONE_ID = 49;   // include/ewal.h's codes
constexpr uint64_t KIND_NONE = 0, KIND_RESTART = 1, KIND_START = 2;
// enode_result.action
constexpr int32_t NONE = 0, RESTARTED = 1, RESTARTED_SNAP = 2, STARTED = 3, PANICKED = 4;

struct Req {
  uint64_t kind, id, n_src;        // n_src: len(ents) (kind 1) or len(peers) (kind 2)
  uint64_t hs_term, hs_vote, hs_commit;
  bool has_snap;                   // kind 1: snapshot != nil
};

// the Snapshot a RestartNode is given: Index, Term and the lengths of Nodes and RemovedNodes
struct Snap {
  uint64_t index, term, n_nodes, n_removed;
};

// What the five records of a built group hold, but the window (ents_first,
// ents_cap), which is the request's.
struct Node {
  uint64_t id, term, committed, off, nlog, np;
  uint64_t pid[PEERS], match[PEERS], next[PEERS];
  uint64_t unstable, pending;
  uint64_t state, vote, lead, elapsed, voted, granted;
  uint64_t hs_term, hs_vote, hs_commit, prev_lead, prev_state, snapi, applied, soft_dirty;
  uint64_t nrem, rem[REMOVED];
  bool restored;                   // restore returned true: raftLog.snapshot is the request's
};

struct Out {
  int32_t status, action;
};

// r.prs, r.removed and votes of newRaft(id, nil, ...): empty
EWAL_HD inline void empty_sets(Node &n) {
  n.np = 0;
NS_UNROLL
  for (uint32_t k = 0; k < PEERS; ++k) n.pid[k] = n.match[k] = n.next[k] = 0;
  n.nrem = 0;
NS_UNROLL
  for (uint32_t k = 0; k < REMOVED; ++k) n.rem[k] = 0;
  n.restored = false;
}

// The two sets raft.restore rebuilds, for a snapshot with s.Index > committed
// on a fresh node of raft id `id`.  node_at(j) is s.Nodes[j], rem_at(j)
// s.RemovedNodes[j].  False: unsupported, n is not to be used.
template <class NodeAt, class RemAt>
EWAL_HD inline bool restore_sets(Node &n, uint64_t id, const Snap &s, const NodeAt &node_at, const RemAt &rem_at) {
  if (s.n_nodes > MAX_NODES) return false;
  // r.prs: the distinct ids in first-occurrence order; lastIndex() is s.Index
  for (uint64_t j = 0; j < s.n_nodes; ++j) {
    const uint64_t node = node_at(j);
    bool seen = false;
NS_UNROLL
    for (uint32_t k = 0; k < PEERS; ++k) seen = seen || (k < n.np && n.pid[k] == node);
    if (seen) continue;
    if (n.np == PEERS) return false;
NS_UNROLL
    for (uint32_t k = 0; k < PEERS; ++k)
      if (k == n.np) {
        n.pid[k] = node;
        n.match[k] = node == id ? s.index : 0;
        n.next[k] = s.index + 1;
      }
    n.np += 1;
  }
  // r.removed
  for (uint64_t j = 0; j < s.n_removed; ++j) {
    const uint64_t node = rem_at(j);
    bool seen = false;
NS_UNROLL
    for (uint32_t k = 0; k < REMOVED; ++k) seen = seen || (k < n.nrem && n.rem[k] == node);
    if (seen) continue;
    if (n.nrem == REMOVED) return false;
NS_UNROLL
    for (uint32_t k = 0; k < REMOVED; ++k)
      if (k == n.nrem) n.rem[k] = node;
    n.nrem += 1;
  }
  n.restored = true;
  return true;
}

// One request.  On a status other than ST_OK n is not to be used: the group
// stays as it was.  The sets come first and every other field is assigned
// exactly once, after the restore loops, as selects -- keep it so: no field is
// written before the loops and again after them.  The cases that hold this in
// place are tests/node_cases.py's lattice entries that combine a restore with a
// non-zero st (snap_index_1_commit_*, snap_index_ffffffffffffffff_commit_*,
// snap_no_entries, own_id_absent, duplicate_nodes, distinct_nodes_7, nodes_64,
// removed_14) on the device, and node_forms.cpp's "loadState" / "prevHardSt"
// checks on the host.
template <class NodeAt, class RemAt>
EWAL_HD inline Out build(Node &n, const Req &r, const Snap &s, const NodeAt &node_at, const RemAt &rem_at) {
  if (r.kind == KIND_NONE) return Out{ST_OK, NONE};
  if (r.id == 0) return Out{ST_PANIC_NONE_ID, PANICKED};   // panic("cannot use none id")
  empty_sets(n);
  // restore(s) returns false at s.Index <= committed, which is 0 on a fresh node: nothing of s is taken then
  if (r.kind == KIND_RESTART && r.has_snap && s.index != 0 && !restore_sets(n, r.id, s, node_at, rem_at))
    return Out{ST_UNSUPPORTED, PANICKED};
  const bool start = r.kind == KIND_START;
  // newRaft and becomeFollower(0, None); raftLog.restore: offset = applied = s.Index
  const uint64_t off = n.restored ? s.index : 0;
  n.id = r.id;
  n.off = n.applied = n.snapi = off;                 // prevSnapi = raftLog.snapshot.Index
  n.pending = 0;
  n.state = n.lead = n.elapsed = n.voted = n.granted = 0;
  n.prev_lead = n.prev_state = n.soft_dirty = 0;     // prevSoftSt = r.softState()
  // StartNode: raftLog.append(0, ents...) leaves unstable 0, committed = len(ents) without a Step, so r.Commit
  // stays 0 until the first one: the previous HardState is seeded with it.
  // RestartNode: loadState without a clamp, loadEnts (it replaces the entry a restore left); prevHardSt = st
  n.term = n.hs_term = start ? 0 : r.hs_term;
  n.vote = n.hs_vote = start ? 0 : r.hs_vote;
  n.committed = n.hs_commit = start ? r.n_src : r.hs_commit;
  n.nlog = start ? 1 + r.n_src : r.n_src;
  n.unstable = start ? 0 : off + r.n_src;
  return Out{ST_OK, start ? STARTED : n.restored ? RESTARTED_SNAP : RESTARTED};
}

// The five records' words: elead_group g[32], elead_prop_state p[4],
// evote_state v[8], eready_state r[8], econf_state c[16]; reserved words 0.
EWAL_HD inline void words(const Node &n, uint64_t ents_first, uint64_t ents_cap, uint64_t *g, uint64_t *p, uint64_t *v,
                          uint64_t *r, uint64_t *c) {
  g[0] = n.id, g[1] = n.term, g[2] = n.committed, g[3] = n.off, g[4] = n.nlog, g[5] = ents_first, g[6] = n.np;
NS_UNROLL
  for (uint32_t k = 0; k < PEERS; ++k) g[7 + k] = n.pid[k], g[14 + k] = n.match[k], g[21 + k] = n.next[k];
  g[28] = g[29] = g[30] = g[31] = 0;
  p[0] = ents_cap, p[1] = n.unstable, p[2] = n.pending, p[3] = 0;
  v[0] = n.state, v[1] = n.vote, v[2] = n.lead, v[3] = n.elapsed, v[4] = n.voted, v[5] = n.granted, v[6] = v[7] = 0;
  r[0] = n.hs_term, r[1] = n.hs_vote, r[2] = n.hs_commit, r[3] = n.prev_lead, r[4] = n.prev_state, r[5] = n.snapi;
  r[6] = n.applied, r[7] = n.soft_dirty;
  c[0] = n.nrem;
NS_UNROLL
  for (uint32_t k = 0; k < REMOVED; ++k) c[1 + k] = n.rem[k];
  c[15] = 0;
}

// ConfChange{ID: 0, Type: ConfChangeAddNode, NodeID: id, Context: ctx}.Marshal():
// 08 00 10 00 18 v(id) 22 v(len) ctx -- every field is written
constexpr uint32_t CONF_HEAD_MAX = 26;
EWAL_HD inline uint64_t conf_change_size(uint64_t id, uint64_t ctx_len) {
  return 6 + ewal_wire::sov(id) + ewal_wire::sov(ctx_len) + ctx_len;
}
EWAL_HD inline uint8_t *conf_change_head(uint8_t *o, uint64_t id, uint64_t ctx_len) {
  *o++ = 0x08; *o++ = 0x00;
  *o++ = 0x10; *o++ = 0x00;
  *o++ = 0x18; o = ewal_wire::put_varint(o, id);
  *o++ = 0x22; o = ewal_wire::put_varint(o, ctx_len);
  return o;
}

}  // namespace node_start
