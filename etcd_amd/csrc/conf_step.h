// conf_step.h -- the decisions of the three membership calls
// (econf_batch_device, econf_scan_committed_device, econf_gate_batch_device),
// shared by their kernels (conf_step.hip) and the host check
// (tests/host/conf_forms.cpp).  Plain C++17, no HIP header.
//
//   step()    one request on a State: node.ApplyConfChange's switch
//             (raft/node.go:228-236) with raft.addNode / removeNode
//             (raft/raft.go:426-435), setProgress / delProgress (:582-588), the
//             head of raft.Step for a msgDenied (:376-387), and the removed half
//             of raft.restore (:549-552).  A request that panics or is
//             unsupported leaves the State as it found it.
//   decode()  ConfChange.Unmarshal (raft/raftpb/raft.pb.go:705-813).
//   gate()    r.removed[m.From] in front of a step call (raft.go:376-382).
//
// r.prs is the group's first n_peers slots, r.removed the econf_state's first
// n_removed ids in insertion order, r.votes the two masks of the evote_state.
// All arithmetic is Go's uint64 and wraps.
#pragma once
#include <cstdint>

#ifndef EWAL_HD
#ifdef __HIPCC__
#define EWAL_HD __host__ __device__
#else
#define EWAL_HD
#endif
#endif

#ifdef __HIPCC__
#define CS_UNROLL _Pragma("unroll")
#else
#define CS_UNROLL
#endif

namespace conf_step {

constexpr uint32_t PEERS = 7, REMOVED = 14;
// include/ewal.h's codes
constexpr int32_t ST_OK = 0, ST_EOF = 2, ST_WRONG_TYPE = 7, ST_ENTRY_TYPE = 8, ST_PANIC_BOUNDS = 33,
                  ST_NONTERMINATING = 37, ST_PANIC_CONF_TYPE = 47, ST_UNSUPPORTED = 48;
// econf_req.kind
constexpr uint64_t KIND_ADD = 1, KIND_REMOVE = 2, KIND_DENIED = 3, KIND_RELOAD = 4;
// econf_result.action
constexpr int32_t NOT_STEPPED = 0, ADDED = 1, REMOVED_NODE = 2, DENIED_BACK = 3, STOPPED = 4, RELOADED = 5,
                  PANICKED = 6;
// econf_gate_result.action
constexpr int32_t G_PASS = 1, G_DENIED = 2, G_DROPPED = 3;
constexpr uint64_t CANDIDATE = 1;                     // raft.StateCandidate
constexpr uint64_t MSG_DENIED = 8;                    // raft.msgDenied (raft/raft.go:17-34)

// What the requests read and write of a group: of its elead_group id, term,
// log_offset, nlog, n_peers and the three peer arrays; pending_conf; the
// evote_state's state and masks; soft_dirty; the econf_state.
struct State {
  uint64_t id, term, off, nlog, np;
  uint64_t pid[PEERS], match[PEERS], next[PEERS];
  uint64_t pending;
  uint64_t rstate, voted, granted;
  uint64_t dirty;
  uint64_t nrem, rem[REMOVED];
};

struct Out {
  int32_t status, action;
  uint64_t n_msgs;                 // 0 or 1: the msgDenied to the request's node
};

EWAL_HD inline bool is_removed(const State &s, uint64_t id) {
  bool hit = false;
CS_UNROLL
  for (uint32_t k = 0; k < REMOVED; ++k) hit |= k < s.nrem && s.rem[k] == id;
  return hit;
}

// the slot of r.prs[id], -1: no such key
EWAL_HD inline int slot_of(const State &s, uint64_t id) {
  int slot = -1;
CS_UNROLL
  for (int k = (int)PEERS - 1; k >= 0; --k)
    if ((uint64_t)k < s.np && s.pid[k] == id) slot = k;
  return slot;
}

// removed[id] = true.  False: a 15th id.
EWAL_HD inline bool add_removed(State &s, uint64_t id) {
  if (is_removed(s, id)) return true;
  if (s.nrem >= REMOVED) return false;
CS_UNROLL
  for (uint32_t k = 0; k < REMOVED; ++k)
    if (k == s.nrem) s.rem[k] = id;
  s.nrem += 1;
  if (id == s.id) s.dirty = 1;                        // ShouldStop changed
  return true;
}

// bits [0, slot) stay, the bits above slot move down by one
EWAL_HD inline uint64_t drop_bit(uint64_t m, uint32_t slot) {
  const uint64_t low = m & ((1ull << slot) - 1);
  return low | ((m >> (slot + 1)) << slot);
}

EWAL_HD inline Out fail(int32_t status) { return Out{status, PANICKED, 0}; }

// One request.  u64_at(j) is word j of the RemovedNodes range of the group's
// snapshot, n_snap_removed its length (kind 4 only).
template <class U64At>
EWAL_HD inline Out step(State &s, uint64_t kind, uint64_t node, uint64_t n_snap_removed, const U64At &u64_at) {
  if (s.np > PEERS) return fail(ST_UNSUPPORTED);
  if (kind == KIND_ADD) {                             // setProgress(node, 0, lastIndex() + 1); pendingConf = false
    const uint64_t next = s.nlog - 1 + s.off + 1;
    int slot = slot_of(s, node);
    if (slot < 0) {
      if (s.np == PEERS) return fail(ST_UNSUPPORTED);
      slot = (int)s.np;
      s.np += 1;
      s.dirty = 1;                                    // SoftState.Nodes changed
    }
CS_UNROLL
    for (int k = 0; k < (int)PEERS; ++k)
      if (k == slot) {
        s.pid[k] = node;
        s.match[k] = 0;
        s.next[k] = next;
      }
    s.pending = 0;
    return Out{ST_OK, ADDED, 0};
  }
  if (kind == KIND_REMOVE) {                          // delProgress(node); pendingConf = false; removed[node] = true
    const int slot = slot_of(s, node);
    if (slot >= 0 && s.rstate == CANDIDATE && ((s.voted >> slot) & 1)) return fail(ST_UNSUPPORTED);
    if (!is_removed(s, node) && s.nrem >= REMOVED) return fail(ST_UNSUPPORTED);
    if (slot >= 0) {
CS_UNROLL
      for (int k = 0; k < (int)PEERS; ++k) {
        if (k < slot || (uint64_t)k >= s.np) continue;
        const int j = k + 1 < (int)PEERS ? k + 1 : k;
        const bool has = (uint64_t)k + 1 < s.np;      // false: the freed slot, zeroed
        s.pid[k] = has ? s.pid[j] : 0;
        s.match[k] = has ? s.match[j] : 0;
        s.next[k] = has ? s.next[j] : 0;
      }
      s.np -= 1;
      s.voted = drop_bit(s.voted, (uint32_t)slot);
      s.granted = drop_bit(s.granted, (uint32_t)slot);
      s.dirty = 1;
    }
    s.pending = 0;
    (void)add_removed(s, node);
    return Out{ST_OK, REMOVED_NODE, 0};
  }
  if (kind == KIND_DENIED) {                          // Step(Message{Type: msgDenied, From: node}), raft.go:376-387
    if (is_removed(s, node)) return Out{ST_OK, DENIED_BACK, node != s.id ? 1ull : 0ull};
    if (!add_removed(s, s.id)) return fail(ST_UNSUPPORTED);
    return Out{ST_OK, STOPPED, 0};
  }
  if (kind == KIND_RELOAD) {                          // r.removed = make(...); for _, n := range s.RemovedNodes
    State t = s;
    t.nrem = 0;
    for (uint64_t j = 0; j < n_snap_removed; ++j) {
      const uint64_t dirty = t.dirty;
      if (!add_removed(t, u64_at(j))) return fail(ST_UNSUPPORTED);
      t.dirty = dirty;
    }
CS_UNROLL
    for (uint32_t k = 0; k < REMOVED; ++k)
      if (k >= t.nrem) t.rem[k] = 0;
    if (is_removed(t, s.id) != is_removed(s, s.id)) t.dirty = 1;
    s = t;
    return Out{ST_OK, RELOADED, 0};
  }
  return fail(ST_PANIC_CONF_TYPE);                    // panic("unexpected conf type"), node.go:235
}

// ---- ConfChange.Unmarshal ---------------------------------------------------
struct ConfChange {
  uint64_t id, node;
  int32_t type;
};

// one varint OR-ed into *v as the generated code does; bits: the width of the field's Go type
EWAL_HD inline int32_t rd_var(const uint8_t *p, int64_t &i, int64_t l, uint64_t *v, uint32_t bits) {
  for (uint32_t shift = 0;; shift += 7) {
    if (i >= l) return ST_EOF;
    const uint8_t b = p[i++];
    if (shift < bits) *v |= (uint64_t)(b & 0x7F) << shift;
    if (b < 0x80) return ST_OK;
  }
}

// skip(p, l, &n) is proto.Skip over p[0, l): 0 and the field's length, or the
// class of its error.
template <class Skip>
EWAL_HD inline int32_t decode(const uint8_t *p, int64_t l, const Skip &skip, ConfChange *cc) {
  uint64_t id = 0, type = 0, node = 0;
  int32_t st = ST_OK;
  int64_t i = 0;
  while (i < l && st == ST_OK) {
    uint64_t wire = 0;
    if (rd_var(p, i, l, &wire, 64)) {
      st = ST_EOF;
      break;
    }
    const uint32_t fn = (uint32_t)(wire >> 3);        // int32(wire >> 3)
    const uint32_t wt = (uint32_t)(wire & 7);
    if (fn >= 1 && fn <= 3) {
      if (wt != 0) st = ST_WRONG_TYPE;
      else st = rd_var(p, i, l, fn == 1 ? &id : fn == 2 ? &type : &node, fn == 2 ? 32 : 64);
    } else if (fn == 4) {
      uint64_t bl = 0;
      if (wt != 2) st = ST_WRONG_TYPE;
      else if (rd_var(p, i, l, &bl, 64)) st = ST_EOF;
      else {
        const int64_t post = (int64_t)((uint64_t)i + bl);
        if (post > l) st = ST_EOF;
        else if (post < i) st = ST_PANIC_BOUNDS;      // data[index:postIndex] with postIndex < index
        else i = post;
      }
    } else {                                          // index -= sizeOfWire; Skip(data[index:])
      int64_t sow = 0;
      uint64_t w = wire;
      do {
        ++sow;
        w >>= 7;
      } while (w);
      i -= sow;
      int64_t skippy = 0;
      st = skip(p + i, l - i, skippy);
      if (st == ST_OK) {
        const int64_t hi = (int64_t)((uint64_t)i + (uint64_t)skippy);
        if (hi > l) st = ST_EOF;
        else if (hi < i) st = ST_PANIC_BOUNDS;
        else if (skippy == 0) st = ST_NONTERMINATING;
        else i = hi;
      }
    }
  }
  cc->id = id;
  cc->type = (int32_t)(uint32_t)type;
  cc->node = node;
  return st;
}

// econf_req.kind of a decoded ConfChange: Type + 1 (ConfChangeAddNode = 0, ConfChangeRemoveNode = 1)
EWAL_HD inline uint64_t kind_of(const ConfChange &cc) { return (uint64_t)(uint32_t)cc.type + 1; }

// ---- the gate -----------------------------------------------------------------
// removed: the group's econf_state words {n_removed, removed[14]}.
EWAL_HD inline int32_t gate(const uint64_t *removed, uint64_t id, uint64_t from) {
  bool hit = false;
CS_UNROLL
  for (uint32_t k = 0; k < REMOVED; ++k) hit |= k < removed[0] && removed[1 + k] == from;
  return !hit ? G_PASS : from != id ? G_DENIED : G_DROPPED;
}

}  // namespace conf_step
