// follow_step.h -- the decisions of the batched follower step
// (efollow_step_batch_device), shared by its kernels (follow_step.hip) and the
// host check (tests/host/follow_forms.cpp).  Plain C++17, no HIP header.
//
// step() is the SERIAL step of one msgApp or msgSnap on a raft group: raft.Step's
// term switch (raft/raft.go:393-405), the msgApp and msgSnap cases of
// stepFollower (:504-510) and stepCandidate (:476-481) -- stepLeader has none --,
// handleAppendEntries (:410-416), handleSnapshot (:418-424), raft.restore
// (:535-554) and, from raft/log.go, maybeAppend, findConflict, append,
// matchTerm, at, slice, isOutOfBounds, lastIndex and restore, restated on
// uint64 arithmetic that wraps as Go's does, with every panic.  reset and
// becomeFollower are vote_step.h's, the group in registers is
// lead_prop_step.h's State: neither is restated here.
//
// step() moves no entry.  It says which suffix of the message's entries goes
// where (Out::app_k, n_app, dst_pos); the copy is the caller's, and so is the
// log's view afterwards: the terms come through a functor TermAt(pos), pos a
// position in ents, that answers for the suffix a record of the same run
// appended (or for the one entry a restore left) from the SOURCE -- Overlay
// below says which positions those are.  run_step() is step() under the rules
// of a run: after a panic the rest is NOT_STEPPED, after a record that appended
// or restored every later record that carries entries or a snapshot is
// DEFERRED, and with it the rest of the run -- so one overlay is all a run
// ever needs.
#pragma once
#include "vote_step.h"

namespace follow_step {

namespace lp = lead_prop;
namespace vs = vote_step;

constexpr uint64_t KIND_APP = 3, KIND_SNAP = 7, MSG_APP_RESP = 4;   // raft.msgApp, msgSnap, msgAppResp
constexpr int32_t ST_PANIC_COMMITTED_CONFLICT = 38;
constexpr uint64_t MAX_NODES = 64;                   // the longest Snapshot.Nodes a restore reads
// efollow_result.action
constexpr int32_t NOT_STEPPED = 0, IGNORED = 1, NO_CASE = 2, APPENDED = 3, REJECTED = 4, RESTORED = 5, SNAP_STALE = 6,
                  DEFERRED = 7, PANICKED = 8;
constexpr int32_t FLAG_TERM_SWITCH = 1, FLAG_CONCEDED = 2;

struct Rec {
  uint64_t kind, from, term, index, log_term, commit, n_ents;
};

// the message's Snapshot: Index, Term and the length of Nodes
struct Snap {
  uint64_t index, term, n_nodes;
};

// the words of the eready_state record a restore writes
struct Ready {
  uint64_t applied, soft_dirty;
};

struct Out {
  int32_t status, action, flags;
  uint64_t n_msgs;                 // 0 or 1: the msgAppResp
  uint64_t resp_index;
  bool resp_reject;
  uint64_t conflict;               // findConflict's ci
  uint64_t app_k, n_app, dst_pos;  // Entries[app_k:] went to ents[dst_pos:]
  bool restored;
};

// What a run has done to its log that memory does not show yet: positions
// [pos, pos + n) hold the source's entries [src, src + n), or (restored) the
// log is the one entry {Term: term}.
struct Overlay {
  uint64_t pos, n, src, term;
  bool restored;
  EWAL_HD inline bool grown() const { return restored || n != 0; }
};

EWAL_HD inline Out blank(int32_t status, int32_t action) {
  Out o;
  o.status = status;
  o.action = action;
  o.flags = 0;
  o.n_msgs = 0;
  o.resp_index = 0;
  o.resp_reject = false;
  o.conflict = o.app_k = o.n_app = o.dst_pos = 0;
  o.restored = false;
  return o;
}

// handleAppendEntries.  src_term(k) is Entries[k].Term.
template <class TermAt, class SrcTerm>
EWAL_HD inline void handle_append(lp::State &s, const Rec &r, const TermAt &term_at, const SrcTerm &src_term, Out &o) {
  const uint64_t last = s.nlog - 1 + s.off;          // lastIndex(), uint64 wrap
  o.n_msgs = 1;
  if (r.index < s.off || r.index > last) {           // matchTerm: at(index) is nil
    o.action = REJECTED;
    o.resp_index = r.index;
    o.resp_reject = true;
    return;
  }
  const uint64_t pos = r.index - s.off;
  if (pos >= s.nlog) {                               // at() indexes past ents: lastIndex() wrapped
    o.status = lp::ST_PANIC_BOUNDS;
    return;
  }
  if (term_at(pos) != r.log_term) {
    o.action = REJECTED;
    o.resp_index = r.index;
    o.resp_reject = true;
    return;
  }
  // findConflict(from, ents), by position: the first of the entries inside the
  // log whose term differs, else the first one past lastIndex()
  const uint64_t from = r.index + 1, after = s.nlog - 1 - pos;
  const uint64_t nm = r.n_ents < after ? r.n_ents : after;
  uint64_t kc = nm;
  for (uint64_t k = 0; k < nm; ++k)
    if (term_at(pos + 1 + k) != src_term(k)) {
      kc = k;
      break;
    }
  const uint64_t ci = kc < r.n_ents ? from + kc : 0; // 0 also when from + kc wrapped to 0
  if (ci != 0 && ci <= s.committed) {
    o.status = ST_PANIC_COMMITTED_CONFLICT;
    return;
  }
  if (ci != 0) {                                     // l.append(ci - 1, ents[ci - from:]...)
    o.conflict = ci;
    o.app_k = kc;
    o.n_app = r.n_ents - kc;
    o.dst_pos = ci - s.off;
    s.nlog = ci - s.off + o.n_app;
    if (ci < s.unstable) s.unstable = ci;
  }
  const uint64_t lastnewi = r.index + r.n_ents;
  const uint64_t tocommit = r.commit < lastnewi ? r.commit : lastnewi;
  if (s.committed < tocommit) s.committed = tocommit;
  o.action = APPENDED;
  o.resp_index = s.nlog - 1 + s.off;
}

// handleSnapshot with raft.restore and raftLog.restore.  node_at(k) is
// Snapshot.Nodes[k], k < sn.n_nodes.
template <class NodeAt>
EWAL_HD inline void handle_snapshot(lp::State &s, const vs::Vote &v, Ready &rd, const Snap &sn, const NodeAt &node_at,
                                    Out &o) {
  o.n_msgs = 1;
  if (sn.index <= s.committed) {
    o.action = SNAP_STALE;
    o.resp_index = s.committed;
    return;
  }
  // the votes map is keyed by peer slot: a restore would move the keys under it
  if (sn.n_nodes > MAX_NODES || v.voted != 0) {
    o.status = lp::ST_UNSUPPORTED;
    return;
  }
  uint64_t ids[lp::PEERS];
  uint64_t np = 0;
LP_UNROLL
  for (uint32_t k = 0; k < lp::PEERS; ++k) ids[k] = 0;
  for (uint64_t j = 0; j < sn.n_nodes; ++j) {
    const uint64_t id = node_at(j);
    bool seen = false;
LP_UNROLL
    for (uint32_t k = 0; k < lp::PEERS; ++k) seen = seen || (k < np && ids[k] == id);
    if (seen) continue;
    if (np == lp::PEERS) {
      o.status = lp::ST_UNSUPPORTED;
      return;
    }
LP_UNROLL
    for (uint32_t k = 0; k < lp::PEERS; ++k)
      if (k == np) ids[k] = id;
    ++np;
  }
  bool changed = np != s.np;
LP_UNROLL
  for (uint32_t k = 0; k < lp::PEERS; ++k) changed = changed || (k < np && ids[k] != s.pid[k]);
  // raftLog.restore
  s.nlog = 1;
  s.unstable = sn.index + 1;
  s.committed = sn.index;
  s.off = sn.index;
  rd.applied = sn.index;
  // r.prs = the snapshot's nodes; lastIndex() is s.Index now
LP_UNROLL
  for (uint32_t k = 0; k < lp::PEERS; ++k) {
    const bool in = k < np;
    s.pid[k] = in ? ids[k] : 0;
    s.match[k] = (in && ids[k] == s.id) ? sn.index : 0;
    s.next[k] = in ? sn.index + 1 : 0;
  }
  s.np = np;
  if (changed) rd.soft_dirty = 1;
  o.action = RESTORED;
  o.restored = true;
  o.resp_index = sn.index;
}

// One msgApp or msgSnap on the state its predecessors left.  On a panic s, v
// and rd are as they were.
template <class TermAt, class SrcTerm, class NodeAt>
EWAL_HD inline Out step(lp::State &s, vs::Vote &v, Ready &rd, const Rec &r, const Snap &sn, const TermAt &term_at,
                        const SrcTerm &src_term, const NodeAt &node_at) {
  Out o = blank(lp::ST_OK, PANICKED);
  const lp::State s0 = s;
  const vs::Vote v0 = v;
  const Ready rd0 = rd;
  if (r.term != 0 && r.term > s.term) {
    vs::become_follower(s, v, r.term, r.from);
    o.flags |= FLAG_TERM_SWITCH;
  } else if (r.term != 0 && r.term < s.term) {
    o.action = IGNORED;
    return o;
  }
  if (v.state == vs::LEADER) {
    o.action = NO_CASE;
    return o;
  }
  if (v.state == vs::CANDIDATE) {
    // msgApp concedes at the candidate's own Term, msgSnap at the message's (0 for a local one: Go's quirk)
    vs::become_follower(s, v, r.kind == KIND_APP ? s.term : r.term, r.from);
    o.flags |= FLAG_CONCEDED;
  } else {
    v.elapsed = 0;
    if (r.kind == KIND_APP) v.lead = r.from;         // a msgSnap does not set lead (Go's quirk)
  }
  if (r.kind == KIND_APP)
    handle_append(s, r, term_at, src_term, o);
  else
    handle_snapshot(s, v, rd, sn, node_at, o);
  if (o.status != lp::ST_OK) {
    s = s0;
    v = v0;
    rd = rd0;
    o = blank(o.status, PANICKED);
  }
  return o;
}

// the rules of a run
struct Run {
  bool stopped, deferring;
  Overlay ov;
};

EWAL_HD inline Run run_start() {
  Run run;
  run.stopped = run.deferring = false;
  run.ov.pos = run.ov.n = run.ov.src = run.ov.term = 0;
  run.ov.restored = false;
  return run;
}

// the log's term at pos as the run sees it; Log(pos) reads ents, Src(k) the source array
template <class Log, class Src>
EWAL_HD inline uint64_t overlay_term(const Overlay &ov, uint64_t pos, const Log &log, const Src &src) {
  if (ov.restored) return ov.term;                   // one entry: pos is 0
  if (pos - ov.pos < ov.n) return src(ov.src + (pos - ov.pos));
  return log(pos);
}

// step() for the next record of a run.  src_first: where Entries starts in the source array.
template <class TermAt, class SrcTerm, class NodeAt>
EWAL_HD inline Out run_step(Run &run, lp::State &s, vs::Vote &v, Ready &rd, const Rec &r, uint64_t src_first,
                            const Snap &sn, const TermAt &term_at, const SrcTerm &src_term, const NodeAt &node_at) {
  if (run.stopped) return blank(lp::ST_OK, NOT_STEPPED);
  if (s.np > lp::PEERS) {
    run.stopped = true;
    return blank(lp::ST_UNSUPPORTED, PANICKED);
  }
  if (run.deferring || (run.ov.grown() && (r.n_ents > 0 || r.kind == KIND_SNAP))) {
    run.deferring = true;
    return blank(lp::ST_OK, DEFERRED);
  }
  const Out o = step(s, v, rd, r, sn, term_at, src_term, node_at);
  if (o.status != lp::ST_OK) run.stopped = true;
  if (o.n_app != 0) {
    run.ov.pos = o.dst_pos;
    run.ov.n = o.n_app;
    run.ov.src = src_first + o.app_k;
  }
  if (o.restored) {
    run.ov.restored = true;
    run.ov.term = sn.term;
  }
  return o;
}

}  // namespace follow_step
