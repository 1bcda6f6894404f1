// lead_prop_step.h -- the decisions of the batched leader msgProp / msgBeat
// step (elead_local_batch_device), shared by its kernels (lead_prop.hip) and
// the host check (tests/host/lead_prop_forms.cpp).  Plain C++17, no HIP header.
//
// Two things live here:
//   step()          the SERIAL step of one local message on a State: stepLeader's
//                   msgBeat and msgProp cases (raft/raft.go:441-455) with
//                   bcastHeartbeat / sendHeartbeat (:219-226, :238-246),
//                   appendEntry (:279-285), raftLog.append (raft/log.go:71-75),
//                   progress.update (:71-74), maybeCommit (:248-258) and
//                   bcastAppend / sendAppend (:202-236), restated on uint64
//                   arithmetic that wraps as Go's does, with every panic.
//   prepare() / closed_record() / closed_state()
//                   the CLOSED FORM of record j of a run in the run's start
//                   state: what step() leaves after the run's first j records,
//                   from two counts alone (the proposals and the ConfChange
//                   proposals among records <= j).  Valid on closed() runs only.
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
#define LP_UNROLL _Pragma("unroll")
#else
#define LP_UNROLL
#endif

namespace lead_prop {

constexpr uint32_t PEERS = 7;
constexpr uint64_t MSG_APP = 3, MSG_SNAP = 7;         // raft.msgApp, raft.msgSnap (raft/raft.go:17-34)
constexpr uint64_t KIND_BEAT = 1, KIND_PROP = 2;      // raft.msgBeat, raft.msgProp
constexpr int32_t ENTRY_CONF_CHANGE = 1;              // raftpb.EntryConfChange
// the status codes of include/ewal.h that a local message can get
constexpr int32_t ST_OK = 0, ST_PANIC_BOUNDS = 33, ST_PANIC_NIL_PROGRESS = 39, ST_PANIC_NEED_SNAPSHOT = 40,
                  ST_PANIC_FIRST_ENTRY = 41, ST_UNSUPPORTED = 48;
// elead_local_result.action
constexpr int32_t NOT_STEPPED = 0, BEAT = 1, APPENDED = 2, DROPPED = 3, PANICKED = 4;

// A leader in registers: the elead_group record, its elead_prop_state, and
// what a run adds.  ents[k] for k >= fresh are entries of this call (their
// term is `term`); the older ones are read through the caller's TermAt.
struct State {
  uint64_t id, term, committed, off, nlog, efirst, np;
  uint64_t pid[PEERS], match[PEERS], next[PEERS];
  uint64_t unstable, pending, fresh;
  bool snap_ok;                    // raftLog.snapshot.Term != 0 (needSnapshot does not panic)
};

struct Msg {
  uint64_t type, to, index, log_term, commit, efirst, nents;   // efirst: a position in ents, not in d_ents
};

struct Out {
  int32_t status, action;
  uint64_t n_msgs, index, pos, committed;   // pos: the new entry's position in ents
};

// raftLog.term(i): 0 where at(i) is nil; ST_PANIC_BOUNDS where Go indexes past ents.
template <bool LOAD, class TermAt>
EWAL_HD inline int32_t log_term(const State &s, uint64_t i, const TermAt &term_at, uint64_t *t) {
  const uint64_t last = s.nlog - 1 + s.off;          // lastIndex(), uint64 wrap
  *t = 0;
  if (i < s.off || i > last) return ST_OK;           // isOutOfBounds
  const uint64_t pos = i - s.off;
  if (pos >= s.nlog) return ST_PANIC_BOUNDS;
  if (LOAD) *t = pos >= s.fresh ? s.term : term_at(pos);
  return ST_OK;
}

// raftLog.slice(lo, hi) (raft/log.go:202-210) of a log of nlog entries at
// offset off, as positions in ents: [*first, *first + *n), *n == 0 where Go
// returns nil; ST_PANIC_BOUNDS where Go indexes past ents (only a wrapped
// lastIndex() gets there).
EWAL_HD inline int32_t log_slice(uint64_t off, uint64_t nlog, uint64_t lo, uint64_t hi, uint64_t *first, uint64_t *n) {
  const uint64_t last = nlog - 1 + off;              // lastIndex(), uint64 wrap
  *first = 0;
  *n = 0;
  if (lo >= hi) return ST_OK;
  if (lo < off || lo > last || hi - 1 < off || hi - 1 > last) return ST_OK;   // isOutOfBounds(lo) || isOutOfBounds(hi - 1)
  const uint64_t lo_p = lo - off, hi_p = hi - off;
  if (lo_p > hi_p || hi_p > nlog) return ST_PANIC_BOUNDS;
  *first = lo_p;
  *n = hi_p - lo_p;
  return ST_OK;
}

// sendAppend for a peer whose Progress.next is `next`: the message, or the
// class of Go's panic.  LOAD false: the class alone, no term is read.
template <bool LOAD, class TermAt>
EWAL_HD inline int32_t send_append(const State &s, uint64_t to, uint64_t next, const TermAt &term_at, Msg *m) {
  const uint64_t index = next - 1;
  m->to = to;
  m->index = index;
  m->log_term = 0;
  m->commit = 0;
  m->efirst = 0;
  m->nents = 0;
  if (index < s.off) {                               // needSnapshot
    m->type = MSG_SNAP;
    return s.snap_ok ? ST_OK : ST_PANIC_NEED_SNAPSHOT;
  }
  m->type = MSG_APP;
  m->commit = s.committed;
  const int32_t st = log_term<LOAD>(s, index, term_at, &m->log_term);
  if (st != ST_OK) return st;
  if (next == s.off) return ST_PANIC_FIRST_ENTRY;    // entries(i) with i == offset
  return log_slice(s.off, s.nlog, next, s.nlog - 1 + s.off + 1, &m->efirst, &m->nents);   // slice(next, lastIndex() + 1)
}

EWAL_HD inline uint64_t n_slots(const State &s) { return s.np < PEERS ? s.np : PEERS; }

// the slot of r.prs[r.id], -1: nil
EWAL_HD inline int self_slot(const State &s) {
  int slot = -1;
LP_UNROLL
  for (int k = (int)PEERS - 1; k >= 0; --k)
    if ((uint64_t)k < s.np && s.pid[k] == s.id) slot = k;
  return slot;
}

// the peers a broadcast reaches: slots whose peer_id != id
EWAL_HD inline uint64_t n_others(const State &s) {
  uint64_t c = 0;
LP_UNROLL
  for (uint32_t k = 0; k < PEERS; ++k) c += (k < s.np && s.pid[k] != s.id) ? 1 : 0;
  return c;
}

// the q-th largest (q >= 1) of match[] over the slots < np other than `skip`;
// *found false when there are fewer than q of them
EWAL_HD inline uint64_t kth_largest(const State &s, int skip, uint64_t q, bool *found) {
  uint64_t v = 0;
  bool f = false;
LP_UNROLL
  for (int k = 0; k < (int)PEERS; ++k) {
    uint64_t above = 0, same = 0;
LP_UNROLL
    for (int j = 0; j < (int)PEERS; ++j) {
      const bool in = (uint64_t)j < s.np && j != skip;
      above += (in && s.match[j] > s.match[k]) ? 1 : 0;
      same += (in && s.match[j] == s.match[k]) ? 1 : 0;
    }
    if ((uint64_t)k < s.np && k != skip && above < q && q <= above + same) {
      v = s.match[k];
      f = true;
    }
  }
  *found = f;
  return v;
}

// msgBeat: bcastHeartbeat.  Nothing changes and nothing can panic.
template <bool EMIT, class Sink>
EWAL_HD inline Out step_beat(const State &s, Sink &sink) {
  Out o;
  o.status = ST_OK;
  o.action = BEAT;
  o.index = 0;
  o.pos = 0;
  o.committed = s.committed;
  uint64_t j = 0;
LP_UNROLL
  for (uint32_t k = 0; k < PEERS; ++k)
    if (k < s.np && s.pid[k] != s.id) {
      if (EMIT) {
        Msg m;
        m.type = MSG_APP;
        m.to = s.pid[k];
        m.index = m.log_term = m.commit = m.efirst = m.nents = 0;
        sink.msg(j, s, m);
      }
      ++j;
    }
  o.n_msgs = j;
  return o;
}

// msgProp with Entries[0].Type == etype.  On a panic s is as it was.  EMIT:
// the entry and the messages go to the sink, after the last check.
template <bool EMIT, class TermAt, class Sink>
EWAL_HD inline Out step_prop(State &s, int32_t etype, const TermAt &term_at, Sink &sink) {
  Out o;
  o.status = ST_OK;
  o.action = DROPPED;
  o.n_msgs = 0;
  o.index = 0;
  o.pos = 0;
  o.committed = s.committed;
  if (etype == ENTRY_CONF_CHANGE && s.pending != 0) return o;
  const State before = s;
  o.action = PANICKED;
  if (etype == ENTRY_CONF_CHANGE) s.pending = 1;
  // appendEntry: e.Term = r.Term, e.Index = lastIndex() + 1
  const uint64_t last = s.nlog - 1 + s.off, index = last + 1;
  // raftLog.append(last, e): ents = append(slice(offset, last + 1), e)
  const bool nil = s.off >= index || s.off > last;   // lo >= hi, or isOutOfBounds(lo) (that of hi - 1 implies it)
  if (!nil && index - s.off > s.nlog) {              // ents[0 : hi - offset] past ents
    s = before;
    o.status = ST_PANIC_BOUNDS;
    return o;
  }
  s.nlog = nil ? 1 : s.nlog + 1;
  if (nil) s.fresh = 0;
  if (index < s.unstable) s.unstable = index;        // min(unstable, after + 1)
  const uint64_t pos = s.nlog - 1;
  // r.prs[r.id].update(lastIndex())
  const int self = self_slot(s);
  if (self < 0) {
    s = before;
    o.status = ST_PANIC_NIL_PROGRESS;
    return o;
  }
  const uint64_t nlast = s.nlog - 1 + s.off;
LP_UNROLL
  for (int k = 0; k < (int)PEERS; ++k)
    if (k == self) {
      s.match[k] = nlast;
      s.next[k] = nlast + 1;
    }
  // maybeCommit, result ignored
  bool found = false;
  const uint64_t mci = kth_largest(s, -1, s.np / 2 + 1, &found);   // np >= 1 here: always found
  if (found && mci > s.committed) {
    uint64_t t = 0;
    o.status = log_term<true>(s, mci, term_at, &t);
    if (o.status != ST_OK) {
      s = before;
      return o;
    }
    if (t == s.term) s.committed = mci;
  }
  // bcastAppend: would its k-th message panic?  (arithmetic alone)
  uint64_t cnt = 0;
LP_UNROLL
  for (uint32_t k = 0; k < PEERS; ++k)
    if (k < s.np && s.pid[k] != s.id && o.status == ST_OK) {
      Msg m;
      o.status = send_append<false>(s, s.pid[k], s.next[k], term_at, &m);
      ++cnt;
    }
  if (o.status != ST_OK) {
    s = before;
    return o;
  }
  if (EMIT) {
    sink.entry(pos, s.term, index);
    uint64_t j = 0;
LP_UNROLL
    for (uint32_t k = 0; k < PEERS; ++k)
      if (k < s.np && s.pid[k] != s.id) {
        Msg m;
        (void)send_append<true>(s, s.pid[k], s.next[k], term_at, &m);
        sink.msg(j, s, m);
        ++j;
      }
  }
  o.action = APPENDED;
  o.n_msgs = cnt;
  o.index = index;
  o.pos = pos;
  o.committed = s.committed;
  return o;
}

// One local message on the state its predecessors left.
template <bool EMIT, class TermAt, class Sink>
EWAL_HD inline Out step(State &s, uint64_t kind, int32_t etype, const TermAt &term_at, Sink &sink) {
  if (kind == KIND_BEAT) return step_beat<EMIT>(s, sink);
  return step_prop<EMIT>(s, etype, term_at, sink);
}

// ---- the closed form ---------------------------------------------------------

// What a run's records share: taken from the run's START state.
struct Run {
  bool closed;        // the closed form holds for every record of the run
  int self;           // prs[id]'s slot
  uint64_t last0;     // lastIndex() at the start
  uint64_t lo, hi;    // the q-th / (q-1)-th largest match of the OTHER peers
  bool hi_inf;        // q == 1: there is no (q-1)-th
  uint64_t others;    // the messages of a broadcast
};

// The run's constants, and whether the closed form may be used: at most 7
// peers with id among them, a non-empty log, a non-zero term (term(i) == 0 ==
// Term would commit indexes outside the log), no uint64 wrap within 2^32
// appends, and no peer whose sendAppend panics (a broadcast's panics depend on
// the start state alone).
EWAL_HD inline Run prepare(const State &s) {
  Run r;
  r.self = self_slot(s);
  r.last0 = s.nlog - 1 + s.off;
  r.others = n_others(s);
  const uint64_t q = s.np / 2 + 1;
  bool f_lo = false, f_hi = false;
  r.lo = kth_largest(s, r.self, q, &f_lo);
  if (!f_lo) r.lo = 0;
  r.hi_inf = q == 1;
  r.hi = r.hi_inf ? 0 : kth_largest(s, r.self, q - 1, &f_hi);
  if (!r.hi_inf && !f_hi) r.hi_inf = true;           // cannot happen with id among <= 7 peers
  const uint64_t end = s.off + s.nlog;
  bool ok = s.np <= PEERS && r.self >= 0 && s.nlog >= 1 && s.term != 0 && end >= s.off &&
            end < 0xFFFFFFFF00000000ull && s.fresh >= s.nlog;
  if (ok) {
    State t = s;
    t.nlog = s.nlog + 1;
    auto none = [](uint64_t) -> uint64_t { return 0; };
LP_UNROLL
    for (uint32_t k = 0; k < PEERS; ++k)
      if (k < s.np && s.pid[k] != s.id) {
        Msg m;
        ok = ok && send_append<false>(t, s.pid[k], s.next[k], none, &m) == ST_OK;
      }
  }
  r.closed = ok;
  return r;
}

// whether some sendAppend of the group would look at the snapshot (index < offset)
EWAL_HD inline bool wants_snapshot(const State &s) {
  bool w = false;
LP_UNROLL
  for (uint32_t k = 0; k < PEERS; ++k) w = w || (k < s.np && s.pid[k] != s.id && s.next[k] - 1 < s.off);
  return w;
}

// The accepted proposals among a run's records <= j, from the proposals
// (nprops) and the ConfChange proposals (ncc) among them: every other
// proposal, and the first ConfChange unless pendingConf was set at the start.
EWAL_HD inline uint64_t accepted_upto(const State &s0, uint64_t nprops, uint64_t ncc) {
  return nprops - ncc + ((s0.pending == 0 && ncc > 0) ? 1 : 0);
}

// whether record j itself, a proposal, is accepted (ncc counts it when it is a ConfChange)
EWAL_HD inline bool accepted(const State &s0, int32_t etype, uint64_t ncc) {
  return etype != ENTRY_CONF_CHANGE || (s0.pending == 0 && ncc == 1);
}

// The state after the first `a` accepted proposals of a closed run, `cc`: a
// ConfChange was among the run's records so far.
//   index_a = last0 + a, at position nlog0 + a - 1
//   mci_a   = median(lo, index_a, hi) -- the q-th largest match once prs[id] is index_a
//   mci_a is monotone in a, and it commits exactly when its term is Term:
//     hi > last0:  term(mci_a) == Term iff last0 < mci_a <= index_a iff lo <= index_a
//                  (past index_a the term is 0); a failing a has only failing predecessors
//     hi <= last0: mci_a == hi for every a: the old log's term decides once
template <class TermAt>
EWAL_HD inline State closed_state(const State &s0, const Run &r, uint64_t a, bool cc, const TermAt &term_at) {
  State s = s0;
  if (a == 0) return s;
  const uint64_t index = r.last0 + a;
  s.nlog = s0.nlog + a;
  if (r.last0 + 1 < s.unstable) s.unstable = r.last0 + 1;
  if (cc) s.pending = 1;
LP_UNROLL
  for (int k = 0; k < (int)PEERS; ++k)
    if (k == r.self) {
      s.match[k] = index;
      s.next[k] = index + 1;
    }
  if (r.hi_inf || r.hi > r.last0) {
    if (r.lo <= index) {
      const uint64_t mci = (!r.hi_inf && r.hi < index) ? r.hi : index;
      if (mci > s.committed) s.committed = mci;
    }
  } else if (r.hi > s.committed && r.hi >= s0.off) {
    if (term_at(r.hi - s0.off) == s0.term) s.committed = r.hi;
  }
  return s;
}

// Record j of a closed run: nprops / ncc count the proposals / ConfChange
// proposals among the run's records <= j (j included).  EMIT: the entry and
// the messages go to the sink.
template <bool EMIT, class TermAt, class Sink>
EWAL_HD inline Out closed_record(const State &s0, const Run &r, uint64_t kind, int32_t etype, uint64_t nprops,
                                 uint64_t ncc, const TermAt &term_at, Sink &sink) {
  const uint64_t a = accepted_upto(s0, nprops, ncc);
  const State s = closed_state(s0, r, a, ncc > 0, term_at);
  if (kind == KIND_BEAT) return step_beat<EMIT>(s, sink);
  Out o;
  o.status = ST_OK;
  o.action = DROPPED;
  o.n_msgs = 0;
  o.index = 0;
  o.pos = 0;
  o.committed = s.committed;
  if (!accepted(s0, etype, ncc)) return o;
  o.action = APPENDED;
  o.n_msgs = r.others;
  o.index = r.last0 + a;
  o.pos = s.nlog - 1;
  if (EMIT) {
    sink.entry(o.pos, s.term, o.index);
    uint64_t j = 0;
LP_UNROLL
    for (uint32_t k = 0; k < PEERS; ++k)
      if (k < s.np && s.pid[k] != s.id) {
        Msg m;
        (void)send_append<true>(s, s.pid[k], s.next[k], term_at, &m);
        sink.msg(j, s, m);
        ++j;
      }
  }
  return o;
}

}  // namespace lead_prop
