// vote_step.h -- the decisions of the batched election step
// (evote_step_batch_device), shared by its kernels (vote_step.hip) and the
// host check (tests/host/vote_step_forms.cpp).  Plain C++17, no HIP header.
//
// step() is the SERIAL step of one election message on a raft group: raft.Step
// (raft/raft.go:372-408) for msgHup, msgVote and msgVoteResp, the msgVote case
// of stepFollower / stepCandidate / stepLeader (:467-468, :482-483, :511-518),
// stepCandidate's msgVoteResp case (:484-492), campaign (:358-370), poll
// (:177-187), reset (:260-273), becomeFollower / becomeCandidate / becomeLeader
// (:309-349) and raftLog.isUpToDate (raft/log.go:136-139), restated on uint64
// arithmetic that wraps as Go's does, with every panic.  becomeLeader's
// appendEntry and the winner's bcastAppend are lead_prop_step.h's step_prop:
// they are not restated here.
//
// The log's terms and types come through two functors, TermAt(pos) and
// TypeAt(pos), pos a position in ents.  An entry that an earlier record of the
// same run appended keeps the term of ITS election, which a later record's
// Term has left behind, so lead_prop's "positions >= fresh carry s.term" holds
// only within one step_prop: step() keeps s.fresh == s.nlog outside it, the
// functors answer for the run's own entries (Run below says which they are),
// and the caller notes every append with Run::note.
#pragma once
#include "lead_prop_step.h"

namespace vote_step {

namespace lp = lead_prop;

constexpr uint64_t KIND_HUP = 0, KIND_VOTE = 5, KIND_VOTE_RESP = 6;   // raft.msgHup, msgVote, msgVoteResp
constexpr uint64_t FOLLOWER = 0, CANDIDATE = 1, LEADER = 2;          // raft.StateType
constexpr int32_t ST_PANIC_LEADER_TO_CANDIDATE = 42, ST_PANIC_NIL_ENTRY = 43, ST_PANIC_DOUBLE_CONF = 44;
// evote_result.action
constexpr int32_t NOT_STEPPED = 0, IGNORED = 1, GRANTED = 2, REJECTED = 3, CAMPAIGNED = 4, WON = 5, LOST = 6,
                  POLLED = 7, NO_CASE = 8, PANICKED = 9;
constexpr int32_t FLAG_TERM_SWITCH = 1;

// the evote_state record
struct Vote {
  uint64_t state, vote, lead, elapsed, voted, granted;
};

struct Rec {
  uint64_t kind, from, term, index, log_term;
  bool reject;
};

struct Out {
  int32_t status, action, flags;
  uint64_t n_msgs;
  bool appended;        // becomeLeader's entry went to position pos with the term s.term
  uint64_t pos;
};

// Which entries are the run's own: positions >= first, the k-th of them
// appended by the run's k-th append.  An append that leaves a log of one entry
// replaced the log (raftLog.append on a nil slice): the run's entries start
// over at position 0.
struct Run {
  uint64_t first;
  EWAL_HD inline void note(const lp::State &s, const Out &o) {
    if (o.appended && s.nlog == 1) first = 0;
  }
};

EWAL_HD inline uint32_t popcount(uint64_t x) { return (uint32_t)__builtin_popcountll((unsigned long long)x); }

// the slot of r.prs[id] among the first n_peers, -1: nil
EWAL_HD inline int slot_of(const lp::State &s, uint64_t id) {
  int slot = -1;
LP_UNROLL
  for (int k = (int)lp::PEERS - 1; k >= 0; --k)
    if ((uint64_t)k < s.np && s.pid[k] == id) slot = k;
  return slot;
}

// raft.reset (raft.go:260-273)
EWAL_HD inline void reset(lp::State &s, Vote &v, uint64_t term) {
  s.term = term;
  v.lead = 0;
  v.vote = 0;
  v.elapsed = 0;
  v.voted = 0;
  v.granted = 0;
  const uint64_t last = s.nlog - 1 + s.off;
LP_UNROLL
  for (uint32_t k = 0; k < lp::PEERS; ++k)
    if (k < s.np) {
      s.match[k] = s.pid[k] == s.id ? last : 0;
      s.next[k] = last + 1;
    }
  s.pending = 0;
}

EWAL_HD inline void become_follower(lp::State &s, Vote &v, uint64_t term, uint64_t lead) {
  reset(s, v, term);
  v.lead = lead;
  v.state = FOLLOWER;
}

// poll(id, grant) for the peer in `slot`: only its first answer counts; returns granted
EWAL_HD inline uint32_t poll(Vote &v, int slot, bool grant) {
  const uint64_t bit = 1ull << slot;
  if (!(v.voted & bit)) {
    v.voted |= bit;
    if (grant) v.granted |= bit;
  }
  return popcount(v.granted);
}

// becomeLeader (raft.go:329-349), called on a candidate, and the broadcast that
// follows it in stepCandidate (campaign's winner has nobody to send to): reset,
// the scan of entries(committed + 1) for EntryConfChange, then step_prop's
// appendEntry + bcastAppend.  On a panic s and v are NOT restored: step() does.
template <bool EMIT, class TermAt, class TypeAt, class Sink>
EWAL_HD inline void become_leader(lp::State &s, Vote &v, const TermAt &term_at, const TypeAt &type_at, Sink &sink,
                                  Out &o) {
  reset(s, v, s.term);
  v.lead = s.id;
  v.state = LEADER;
  const uint64_t i = s.committed + 1;
  if (i == s.off) {                                  // entries(i) with i == offset
    o.status = lp::ST_PANIC_FIRST_ENTRY;
    return;
  }
  const uint64_t last = s.nlog - 1 + s.off, hi = last + 1;
  if (i < hi && !(i < s.off || i > last)) {          // slice(i, lastIndex() + 1) is not nil
    const uint64_t lo_p = i - s.off, hi_p = hi - s.off;
    if (lo_p > hi_p || hi_p > s.nlog) {
      o.status = lp::ST_PANIC_BOUNDS;
      return;
    }
    for (uint64_t p = lo_p; p < hi_p; ++p) {
      if (type_at(p) != lp::ENTRY_CONF_CHANGE) continue;
      if (s.pending != 0) {
        o.status = ST_PANIC_DOUBLE_CONF;
        return;
      }
      s.pending = 1;
    }
  }
  s.fresh = s.nlog;
  const lp::Out a = lp::step_prop<EMIT>(s, 0, term_at, sink);
  s.fresh = s.nlog;
  o.status = a.status;
  if (a.status != lp::ST_OK) return;
  o.n_msgs = a.n_msgs;
  o.appended = true;
  o.pos = a.pos;
}

// One election message on the state its predecessors left.  On a panic s and
// v are as they were and nothing went to the sink.  EMIT: the entry and the
// messages go to the sink, after the last check; sink.msg(j, ...) /
// sink.vote_resp(j, ...) get the record's j-th message.
template <bool EMIT, class TermAt, class TypeAt, class Sink>
EWAL_HD inline Out step(lp::State &s, Vote &v, const Rec &r, const TermAt &term_at, const TypeAt &type_at,
                        Sink &sink) {
  Out o;
  o.status = lp::ST_OK;
  o.action = PANICKED;
  o.flags = 0;
  o.n_msgs = 0;
  o.appended = false;
  o.pos = 0;
  const lp::State s0 = s;
  const Vote v0 = v;
  s.fresh = s.nlog;
  bool win = false, hup = false;
  if (r.kind == KIND_HUP) {
    // campaign(): becomeCandidate, poll(id, true)
    if (v.state == LEADER) {
      o.status = ST_PANIC_LEADER_TO_CANDIDATE;
    } else if (slot_of(s, s.id) < 0) {
      o.status = lp::ST_UNSUPPORTED;                 // not promotable: the self vote has no slot
    } else {
      reset(s, v, s.term + 1);
      v.vote = s.id;
      v.state = CANDIDATE;
      hup = true;
      win = s.np / 2 + 1 == poll(v, slot_of(s, s.id), true);
      o.action = win ? WON : CAMPAIGNED;
    }
  } else {
    bool stepped = true;
    if (r.term != 0 && r.term > s.term) {
      become_follower(s, v, r.term, r.kind == KIND_VOTE ? 0 : r.from);
      o.flags = FLAG_TERM_SWITCH;
    } else if (r.term != 0 && r.term < s.term) {
      o.action = IGNORED;
      stepped = false;
    }
    if (stepped && r.kind == KIND_VOTE) {
      bool grant = false;
      if (v.state == FOLLOWER && (v.vote == 0 || v.vote == r.from)) {
        // isUpToDate: e = at(lastIndex()), dereferenced
        const uint64_t last = s.nlog - 1 + s.off;
        if (last < s.off) {
          o.status = ST_PANIC_NIL_ENTRY;
        } else if (last - s.off >= s.nlog) {
          o.status = lp::ST_PANIC_BOUNDS;            // at() indexes past ents: an empty log at offset 0
        } else {
          const uint64_t et = term_at(last - s.off);
          grant = r.log_term > et || (r.log_term == et && r.index >= last);
        }
      }
      if (o.status == lp::ST_OK) {
        if (grant) {
          v.elapsed = 0;
          v.vote = r.from;
        }
        o.action = grant ? GRANTED : REJECTED;
        o.n_msgs = 1;
        if (EMIT) sink.vote_resp(0, s, r.from, !grant);
      }
    } else if (stepped) {
      if (v.state != CANDIDATE) {
        o.action = NO_CASE;
      } else {
        const int slot = slot_of(s, r.from);
        if (slot < 0) {
          o.status = lp::ST_UNSUPPORTED;             // Go would count it; the mask cannot
        } else {
          const uint32_t gr = poll(v, slot, !r.reject);
          const uint64_t q = s.np / 2 + 1;
          if (q == gr) {
            win = true;                              // becomeLeader, bcastAppend
            o.action = WON;
          } else if (q == popcount(v.voted) - gr) {
            become_follower(s, v, s.term, 0);
            o.action = LOST;
          } else {
            o.action = POLLED;
          }
        }
      }
    }
  }
  // campaign's winner (q() == 1) has nobody to send to: its broadcast is empty,
  // and so is its msgVote fan-out below (nothing can panic after its entry went to the sink)
  if (win) become_leader<EMIT>(s, v, term_at, type_at, sink, o);
  if (hup && o.status == lp::ST_OK) {
    // campaign's msgVote fan-out; then Step's term switch (m.Term == 0: local) and no msgHup case
    const uint64_t others = lp::n_others(s), lasti = s.nlog - 1 + s.off;
    uint64_t lt = 0;
    if (others != 0) o.status = lp::log_term<true>(s, lasti, term_at, &lt);
    if (o.status == lp::ST_OK) {
      if (EMIT) {
        uint64_t j = o.n_msgs;
LP_UNROLL
        for (uint32_t k = 0; k < lp::PEERS; ++k)
          if (k < s.np && s.pid[k] != s.id) {
            lp::Msg m;
            m.type = KIND_VOTE;
            m.to = s.pid[k];
            m.index = lasti;
            m.log_term = lt;
            m.commit = m.efirst = m.nents = 0;
            sink.msg(j, s, m);
            ++j;
          }
      }
      o.n_msgs += others;
    }
  }
  if (o.status != lp::ST_OK) {
    s = s0;
    v = v0;
    o.action = PANICKED;
    o.flags = 0;
    o.n_msgs = 0;
    o.appended = false;
    o.pos = 0;
  }
  return o;
}

}  // namespace vote_step
