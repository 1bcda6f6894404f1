// ready_step.h -- the decisions of the batched Ready (eready_batch_device),
// shared by its kernels (ready_step.hip) and the host check
// (tests/host/ready_forms.cpp).  Plain C++17, no HIP header.
//
// decide() is newReady (raft/node.go:332-348) with containsUpdates (:83-86,
// without its Messages term), the record count of Storage.Save (wal/wal.go:
// 281-288) and what node.run's accept branch (:239-255) leaves, for one group:
// a map from the words of its four records and its snapshot index to flags,
// the two entry views, the HardState triple and the accepted words.  The
// slices are lead_prop_step.h's log_slice.  All arithmetic is Go's uint64.
#pragma once
#include "lead_prop_step.h"

namespace ready_step {

namespace lp = lead_prop;

constexpr int32_t SOFT = 1, HARD = 2, SNAP = 4, UPDATES = 8;   // eready_result.flags
constexpr uint64_t SAVE_ENTRY = 2, SAVE_STATE = 3;              // ewal_save_rec.kind

// what the call reads of a group
struct In {
  uint64_t term, committed, off, nlog;               // elead_group
  uint64_t unstable;                                 // elead_prop_state
  uint64_t state, vote, lead;                        // evote_state
  uint64_t hs_term, hs_vote, hs_commit, plead, pstate, snapi, applied, soft_dirty;   // eready_state
  uint64_t snap_index;                               // raftLog.snapshot.Index
};

struct Out {
  int32_t status, flags;
  uint64_t term, vote, commit;                       // rd.HardState
  uint64_t ents_pos, n_ents;                         // rd.Entries: positions in the group's ents
  uint64_t committed_pos, n_committed;               // rd.CommittedEntries
  uint64_t n_save;                                   // Save's records: the HardState's, then one per entry
  uint64_t lead, state;                              // rd.SoftState
  uint64_t applied, unstable;                        // after resetNextEnts / resetUnstable
};

EWAL_HD inline Out decide(const In &g) {
  Out o;
  o.flags = 0;
  o.term = o.vote = o.commit = 0;
  o.ents_pos = o.n_ents = o.committed_pos = o.n_committed = o.n_save = 0;
  o.lead = o.state = 0;
  o.applied = g.applied;
  o.unstable = g.unstable;
  const uint64_t last = g.nlog - 1 + g.off;          // lastIndex(), uint64 wrap
  // unstableEnts(), then nextEnts()
  uint64_t upos = 0, un = 0, cpos = 0, cn = 0;
  o.status = lp::log_slice(g.off, g.nlog, g.unstable, last + 1, &upos, &un);
  if (o.status == lp::ST_OK && g.committed > g.applied)
    o.status = lp::log_slice(g.off, g.nlog, g.applied + 1, g.committed + 1, &cpos, &cn);
  if (o.status != lp::ST_OK) return o;
  o.ents_pos = upos;
  o.n_ents = un;
  o.committed_pos = cpos;
  o.n_committed = cn;
  if (g.lead != g.plead || g.state != g.pstate || g.soft_dirty != 0) {
    o.flags |= SOFT;
    o.lead = g.lead;
    o.state = g.state;
  }
  // r.HardState with Step's deferred r.Commit = raftLog.committed
  if (g.term != g.hs_term || g.vote != g.hs_vote || g.committed != g.hs_commit) {
    o.term = g.term;
    o.vote = g.vote;
    o.commit = g.committed;
  }
  if ((o.term | o.vote | o.commit) != 0) o.flags |= HARD;      // !IsEmptyHardState
  if (g.snap_index != g.snapi && g.snap_index != 0) o.flags |= SNAP;
  if (o.flags != 0 || un != 0 || cn != 0) o.flags |= UPDATES;
  o.n_save = un + ((o.flags & HARD) ? 1 : 0);
  if (g.committed > g.applied) o.applied = g.committed;
  o.unstable = last + 1;
  return o;
}

// an entry whose Data lies outside d_data (ewal_entry.data_nil == 2): its group is unsupported
EWAL_HD inline bool data_outside(int32_t data_nil) { return data_nil == 2; }

// The seven words of an ewal_save_rec {kind | etype << 32, a, b, c, data_off,
// data_len, data_nil | pad << 32}: SaveState(&HardState{term, vote, commit}) ...
EWAL_HD inline void save_of_state(uint64_t w[7], uint64_t term, uint64_t vote, uint64_t commit) {
  w[0] = SAVE_STATE;
  w[1] = term;
  w[2] = vote;
  w[3] = commit;
  w[4] = w[5] = w[6] = 0;
}

// ... and SaveEntry of the ewal_entry whose five words are e {term, index,
// data_off, data_len, type | data_nil << 32}
EWAL_HD inline void save_of_entry(uint64_t w[7], const uint64_t e[5]) {
  w[0] = SAVE_ENTRY | (e[4] << 32);                  // kind, etype = type
  w[1] = e[0];
  w[2] = e[1];
  w[3] = 0;
  w[4] = e[2];
  w[5] = e[3];
  w[6] = e[4] >> 32;                                 // data_nil, pad 0
}

}  // namespace ready_step
