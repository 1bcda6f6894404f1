// compact_step.h -- the decisions of the batched log compaction
// (ecompact_batch_device), shared by its kernels (compact_step.hip) and the
// host check (tests/host/compact_forms.cpp).  Plain C++17, no HIP header.
//
// decide() is one node.Compact on a raft group (raft/node.go:226-227, 325-330):
// raft.compact (raft/raft.go:522-531) with raftLog.term, raftLog.snap's Index /
// Term and raftLog.compact (raft/log.go:119-124, 156-179) under
// isOutOfAppliedBounds (:219-224), and -- for a request that asks "at applied,
// when due" -- raftLog.shouldCompact (:181-183) with the caller's threshold,
// restated on uint64 arithmetic that wraps as Go's does, with every panic.  The
// group in registers is lead_prop_step.h's State, raftLog.term and
// raftLog.slice are its log_term and log_slice: neither is restated here.
//
// decide() moves no entry and writes no snapshot.  It says what the log
// becomes (Out::index, n_left, shift, unstable) and how the survivors travel to
// the window's base (move_class); the traffic is the caller's.
#pragma once
#include "lead_prop_step.h"

namespace compact_step {

namespace lp = lead_prop;

constexpr int32_t ST_PANIC_COMPACT_APPLIED = 45, ST_PANIC_COMPACT_BOUNDS = 46;
// ecompact_result.action
constexpr int32_t NOT_STEPPED = 0, NOT_DUE = 1, COMPACTED = 2, PANICKED = 3;
constexpr uint64_t AT_APPLIED = 1;                   // ecompact_req.flags bit 0
// how n_left survivors get from position shift to position 0 of the window
constexpr uint32_t MOVE_NONE = 0, MOVE_DISJOINT = 1, MOVE_OVERLAP = 2;

struct Req {
  uint64_t flags, index, threshold;
};

struct Out {
  int32_t status, action;
  uint64_t index, term;            // the snapshot's
  uint64_t n_left, shift;          // len(ents) afterwards; the entries dropped
  uint64_t unstable;               // raftLog.unstable afterwards
};

EWAL_HD inline Out blank(int32_t status, int32_t action) {
  Out o;
  o.status = status;
  o.action = action;
  o.index = o.term = o.n_left = o.shift = o.unstable = 0;
  return o;
}

// source [shift, shift + n_left) and target [0, n_left) share no entry iff shift >= n_left
EWAL_HD inline uint32_t move_class(uint64_t n_left, uint64_t shift) {
  if (shift == 0 || n_left == 0) return MOVE_NONE;
  return shift >= n_left ? MOVE_DISJOINT : MOVE_OVERLAP;
}

// One request on the group s whose raftLog.applied is `applied`.  term_at(pos)
// is ents[pos].Term.  s is not modified: a COMPACTED request's new offset, len
// and unstable are o.index, o.n_left and o.unstable.
template <class TermAt>
EWAL_HD inline Out decide(const lp::State &s, uint64_t applied, const Req &r, const TermAt &term_at) {
  uint64_t index = r.index;
  if (r.flags & AT_APPLIED) {                        // shouldCompact, then EtcdServer.snapshot's index
    if (!(applied - s.off > r.threshold)) return blank(lp::ST_OK, NOT_DUE);
    index = applied;
  }
  if (index > applied) return blank(ST_PANIC_COMPACT_APPLIED, PANICKED);   // raft.compact
  uint64_t term = 0;
  const int32_t st = lp::log_term<true>(s, index, term_at, &term);         // raftLog.term(index)
  if (st != lp::ST_OK) return blank(st, PANICKED);
  if (index < s.off) return blank(ST_PANIC_COMPACT_BOUNDS, PANICKED);      // isOutOfAppliedBounds; > applied is gone
  uint64_t first = 0, n = 0;
  const int32_t sl = lp::log_slice(s.off, s.nlog, index, s.nlog - 1 + s.off + 1, &first, &n);
  if (sl != lp::ST_OK) return blank(sl, PANICKED);
  if (n == 0) return blank(lp::ST_UNSUPPORTED, PANICKED);   // Go's slice is nil: the log would be left empty
  Out o = blank(lp::ST_OK, COMPACTED);
  o.index = index;
  o.term = term;
  o.n_left = n;
  o.shift = first;
  o.unstable = index + 1 > s.unstable ? index + 1 : s.unstable;
  return o;
}

}  // namespace compact_step
